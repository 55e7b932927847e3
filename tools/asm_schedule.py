"""What load / MFMA schedule did the compiler give a kernel?  Reads gfx950 device assembly (the file the build keeps
beside the object, tensor-ops_amd/build.py device_asm, or any `hipcc ... --cuda-device-only -S` / -save-temps output) and
prints, for one named kernel: VGPRs, scratch bytes, the vector-memory loads issued ahead of the first MFMA, and the
`vmcnt` the wave waits for in front of each MFMA -- the number of younger loads that may still be in flight when that
MFMA issues.  A one-shot body shows all its loads up front and a falling vmcnt; a dripped schedule shows a few loads up
front and MFMAs that each wait (vmcnt 0..3) for a load issued a few instructions earlier.  Needs no GPU.

  python tools/asm_schedule.py tensor-ops_amd/build/gemm_small-hip-amdgcn-amd-amdhsa-gfx950.s \\
      gemm_small_pair_kernelIfLi1ELi0ELi16ELi32ELi8E --mfma 32x32x2

The kernel is named by a substring of its (mangled) symbol; exactly one kernel must match.  --mfma restricts the report
to one MFMA shape (the pair kernel holds a 32x32x2 body and a 16x16x4 body): events are then counted from the kernel's
entry, or from behind the last MFMA of ANOTHER shape that precedes the first wanted one, up to the last wanted MFMA --
the bodies of a multi-body kernel are told apart by where their MFMAs sit in the text."""
import argparse
import re
import sys

LOAD = re.compile(r"^(buffer_load_|global_load_|flat_load_|scratch_load_)")
STORE = re.compile(r"^(buffer_store_|global_store_|flat_store_|scratch_store_|buffer_atomic_|global_atomic_|flat_atomic_)")


def kernel_text(lines, pattern):
    """(symbol, [instruction lines]) of the one function whose symbol contains `pattern`"""
    found = []
    name, start = None, 0
    for n, l in enumerate(lines):
        t = l.split(";")[0].strip()
        if t.endswith(":") and " " not in t and not t.startswith(".L") and not t.startswith("."):
            name, start = t[:-1], n
        elif t.startswith(".Lfunc_end") and name:
            if pattern in name:
                found.append((name, start, n))
            name = None
    if len(found) != 1:
        raise SystemExit("%d kernels match %r%s" % (len(found), pattern, "".join("\n  " + f[0] for f in found[:12])))
    name, lo, hi = found[0]
    return name, lines[lo:hi + 1], lines[hi:]


def resources(name, tail):
    """(vgprs, agprs, scratch bytes) from the comment block the compiler prints behind the function"""
    out = {}
    for l in tail[:120]:
        for key, tag in (("NumVgprs", "vgprs"), ("NumAgprs", "agprs"), ("ScratchSize", "scratch")):
            m = re.match(r"\s*;\s*" + key + r":\s*(\d+)", l)
            if m and tag not in out:
                out[tag] = int(m.group(1))
        if len(out) == 3:
            break
    return out.get("vgprs"), out.get("agprs"), out.get("scratch")


def schedule(body, shape=None):
    """events of the stretch of code that holds the MFMAs of `shape` (any shape when None), in text order:
    ("load", mnemonic) / ("mfma", vmcnt in force: the last vmcnt waited for since the previous MFMA, or None)"""
    ins = []
    for l in body:
        t = l.split(";")[0].strip()
        if not t or t.endswith(":") or t.startswith("."):
            continue
        ins.append(t)
    def is_mfma(t):
        return t.startswith("v_mfma_")
    def wanted(t):
        return is_mfma(t) and (shape is None or shape in t.split()[0])
    idx = [n for n, t in enumerate(ins) if wanted(t)]
    if not idx:
        return []
    first, last = idx[0], idx[-1]
    begin = 0
    for n in range(first - 1, -1, -1):   # the body starts behind the previous body's last MFMA (or at the entry)
        if is_mfma(ins[n]) and not wanted(ins[n]):
            begin = n + 1
            break
    ev, vm = [], None
    for n in range(begin, last + 1):
        t = ins[n]
        op = t.split()[0]
        if LOAD.match(op) and "lds" not in op:
            ev.append(("load", op))
        elif STORE.match(op):
            ev.append(("store", op))
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", t)
            if m:
                vm = int(m.group(1))
        elif wanted(t):
            ev.append(("mfma", vm))
            vm = None
    return ev


def report(path, pattern, shape=None):
    lines = open(path).read().split("\n")
    name, body, tail = kernel_text(lines, pattern)
    vg, ag, sc = resources(name, tail)
    ev = schedule(body, shape)
    ahead = 0
    for kind, _ in ev:
        if kind == "mfma":
            break
        ahead += kind == "load"
    order = "".join("L" if k == "load" else "M" if k == "mfma" else "" for k, _ in ev)
    return {"kernel": name, "vgprs": vg, "agprs": ag, "scratch": sc,
            "loads": sum(k == "load" for k, _ in ev), "mfmas": sum(k == "mfma" for k, _ in ev),
            "loads_ahead": ahead, "vmcnt": [v for k, v in ev if k == "mfma"], "order": order}


def runs(order):
    """'LLLLMMLL' -> 'L4 M2 L2'"""
    out = []
    for c in order:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return " ".join("%s%d" % (c, n) for c, n in out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm")
    ap.add_argument("kernel", help="substring of the kernel's symbol")
    ap.add_argument("--mfma", default=None, help="MFMA shape to report, e.g. 32x32x2")
    a = ap.parse_args()
    r = report(a.asm, a.kernel, a.mfma)
    print("kernel   ", r["kernel"])
    print("VGPRs     %s   AGPRs %s   scratch %s bytes" % (r["vgprs"], r["agprs"], r["scratch"]))
    print("loads     %d, of which ahead of the first MFMA: %d" % (r["loads"], r["loads_ahead"]))
    print("MFMAs     %d" % r["mfmas"])
    print("order     " + runs(r["order"]))
    print("vmcnt in front of MFMA 1..%d (- = none since the previous MFMA): %s"
          % (r["mfmas"], ", ".join("-" if v is None else str(v) for v in r["vmcnt"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
