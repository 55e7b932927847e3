"""One line per kernel file: the name, the line count and the sha256 of its gfx950 device assembly.

A refactor that only moves device helpers between headers leaves every file's generated code as it was; two runs -- one on a
copy of the parent tree, one on the branch -- show that, or name the file where it is not so.  Each file is compiled with
tensor-ops_amd/build.py's FLAGS (plus any -D given here: the development defines are -DTOPS_AB_KNOBS
-DTOPS_GEMM_AB_VARIANTS) and `--cuda-device-only -S` into a temporary directory.  Lines naming `__hip_cuid_<hash>` are dropped
before hashing: that id is hashed from the source text and path, so it differs between any two trees.  Nothing else is
filtered and nothing is searched for; no GPU is needed.
usage: device_asm_digest.py [-DNAME ...] [--keep DIR] [csrc/*.hip file names; default: every .hip of build.py's SOURCES]"""
import argparse
import concurrent.futures
import hashlib
import importlib.util
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_mod():
    spec = importlib.util.spec_from_file_location("_tops_build", os.path.join(ROOT, "tensor-ops_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def digest(b, src, defines, tmp, keep):
    out = os.path.join(tmp, src + ".s")
    cmd = [b._hipcc()] + b.FLAGS + defines + ["--cuda-device-only", "-S", "-o", out, "-x", "hip", os.path.join(b.CSRC, src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-3000:])
    with open(out) as f:
        lines = [l for l in f if "__hip_cuid_" not in l]
    text = "".join(lines)
    if keep:   # the filtered text, so that two builds can be diffed
        with open(os.path.join(keep, src + ".s"), "w") as f:
            f.write(text)
    return len(lines), hashlib.sha256(text.encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="*")
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--keep", metavar="DIR")
    a = ap.parse_args()
    b = _build_mod()
    files = [os.path.basename(f) for f in a.files] or [s for s in b.SOURCES if s.endswith(".hip")]
    if a.keep:
        os.makedirs(a.keep, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        jobs = [pool.submit(digest, b, f, ["-D" + d for d in a.defines], tmp, a.keep) for f in files]
        for f, j in zip(files, jobs):
            print("%-24s %8d  %s" % ((f,) + j.result()), flush=True)


if __name__ == "__main__":
    main()
