// fp64 GEMM between the latency-bound and the full-chip regime -- gemm_kwave.hip's design in the reference's own
// element type (`HMat Double`, src/TensorOps/BLAS/HMat.hs:35): C = alpha * A.B (+ bias, activation, act')
//
// One workgroup of four waves per 64x64 output tile, the K loop split over the WAVES: every wave computes the whole
// tile for its own run of 16-deep k-tiles from wave-private LDS images it fills itself by DMA (no barrier in the
// loop), the four partial tiles are added in LDS in wave order, a ragged last k-tile is added by the last wave
// straight from global memory.  The tiled fp64 kernel (gemm_f64.hip) needs 256x128 tiles to keep the L2 behind it and
// fills the chip only from ~2048^2 outputs on (1024^3: 25 TF of 78.6); its mid-size routes split K over workgroups
// with partial products in HBM.
//
// v_mfma_f64_16x16x4_f64: A operand lane l = A[i = l&15][k = l>>4], B operand lane l = B[k = l>>4][j = l&15],
// D: 4 f64 per lane, col = l&15, row = (l>>4) + 4 r.  A wave's 64x64 tile is 4x4 such tiles (128 accumulator
// registers).  A k-tile is consumed in two halves of two MFMA k-steps; lane (x, kg) of half-tile h, step e uses
// k = 8 h + 2 kg + e (A and B agree), so a k-contiguous operand's fragment for a half-tile is ONE ds_read_b128 (its
// image: [x][8 chunks of 2 k], chunk c of row x in slot c ^ (x & 7)), and an m-/n-contiguous operand is read
// row-/column-OWNING from its [k][64] image: lane l15 holds rows 4 l15 .. 4 l15 + 3, two 16-byte reads per k-step.
#include <cstdio>
#include <type_traits>

#include "common.hpp"
#include "devmath.hpp"

namespace to {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

template <int I, int N, class F>
__device__ __forceinline__ void kw64_static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    kw64_static_for<I + 1, N>(f);
  }
}

struct Kw64Args {
  const double* A;
  const double* B;
  double* C;
  int M, N, K;
  long a_sm, a_sk, b_sk, b_sn, c_sm;
  int tiles_m, tiles_n;
  double alpha;
  const double* bias;
  const double* dact;
  const double* cin;   // beta * cin[m * c_sm + n] joins the sum (the layout of C; may BE C: every element is read, then written, by one thread)
  double beta;
  int act, dact_kind;
  int wide;  // 16-byte stores legal (C 16-byte aligned, c_sm and N even)
};

// AMODE: 0 = A k-contiguous (a_sk == 1), 1 = A m-contiguous (a_sm == 1)
// BMODE: 0 = B n-contiguous (b_sn == 1), 1 = B k-contiguous (b_sk == 1)
template <int AMODE, int BMODE, int NW, int NI>
__global__ __launch_bounds__(NW * 64) void gemm_kw64_kernel(Kw64Args g) {
  constexpr int BM = 64, BN = 64, BK = 16, TM = 4, TN = 4, GA = 8, GB = 8;  // GA/GB: 1-KiB DMA pieces per image
  constexpr int IMG = BM * BK;                 // doubles per image (A and B alike)
  constexpr int WAVE_DOUBLES = 2 * NI * IMG;   // a wave's LDS: [NI] A images, [NI] B images
  static_assert(WAVE_DOUBLES >= BM * BN, "the partial tile reuses the wave's images");
  __shared__ __attribute__((aligned(16))) double smem[NW * WAVE_DOUBLES];

  // XCD-aware tile order (as gemm_kw_kernel)
  const int nblk = g.tiles_m * g.tiles_n;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = nblk >> 3, r = nblk & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  int tile_m, tile_n;
  {
    constexpr int R = 4;
    const int band = bid / (R * g.tiles_n);
    const int rows = (g.tiles_m - band * R) < R ? (g.tiles_m - band * R) : R;
    const int in = bid - band * R * g.tiles_n;
    tile_n = in / rows;
    tile_m = band * R + in % rows;
  }
  const long m0 = (long)tile_m * BM, n0 = (long)tile_n * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, kg = lane >> 4;

  f64x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;

  const int KT = g.K / BK;
  const int per = (KT + NW - 1) / NW;
  const int t_begin = wave * per < KT ? wave * per : KT;
  const int t_end = t_begin + per < KT ? t_begin + per : KT;
  const int nT = t_end - t_begin;

  typedef __attribute__((address_space(3))) void* lptr_t;
  const unsigned lds_a = (unsigned)(unsigned long)(lptr_t)(smem + wave * WAVE_DOUBLES);  // [NI][IMG]
  const unsigned lds_b = lds_a + NI * IMG * 8;                                           // [NI][IMG]

  constexpr int RA = 4, RB = 4;  // LDS reads per half k-tile and operand (k-contiguous: one per tile; owning: 2 steps x 2 pairs)
  static_assert(RA + RB + GA + GB <= 2 * TM * TN, "a slot behind every MFMA of the second half");
  // DMA: scalar base + per-lane 32-bit byte offset (gemm_kwave.hip): piece q's offset biased by -(q % 4) KiB, the base
  // by -3 KiB.  A piece is 1 KiB = 128 doubles of the image; lane l fills doubles 128 q + 2 l, + 1.
  unsigned oa[GA], ob[GB];
#pragma unroll
  for (int q = 0; q < GA; ++q) {
    const int f = q * 128 + lane * 2;
    long e;
    if constexpr (AMODE == 1) {
      long m = m0 + f % BM;  // two consecutive rows (M even: a pair is in or out)
      if (m + 2 > g.M) m = g.M - 2;
      e = (long)(f / BM) * g.a_sk + m;
    } else {
      long m = m0 + f / BK;
      const int x = f / BK;
      if (m >= g.M) m = g.M - 1;
      e = m * g.a_sm + 2 * (((f % BK) / 2) ^ (x & 7));
    }
    oa[q] = (unsigned)(e * 8 + 3072 - (q % 4) * 1024);
  }
#pragma unroll
  for (int q = 0; q < GB; ++q) {
    const int f = q * 128 + lane * 2;
    long e;
    if constexpr (BMODE == 0) {
      long n = n0 + f % BN;
      if (n + 2 > g.N) n = g.N - 2;
      e = (long)(f / BN) * g.b_sk + n;
    } else {
      long n = n0 + f / BK;
      const int x = f / BK;
      if (n >= g.N) n = g.N - 1;
      e = n * g.b_sn + 2 * (((f % BK) / 2) ^ (x & 7));
    }
    ob[q] = (unsigned)(e * 8 + 3072 - (q % 4) * 1024);
  }
  const long step_a = (AMODE == 1 ? (long)BK * g.a_sk : BK) * 8, step_b = (BMODE == 0 ? (long)BK * g.b_sk : BK) * 8;  // bytes
  const char* sa = reinterpret_cast<const char*>(g.A) - 3072 + (long)t_begin * step_a;
  const char* sb = reinterpret_cast<const char*>(g.B) - 3072 + (long)t_begin * step_b;
  // (`; @dma K` / `; @rd K` / `; @images` / `; @advance`: which k-tile's image, relative to the loop's current tile t, an
  //  access touches -- comments for tools/asm_inflight_check.py, see gemm_kwave.hip)
#define KW_DMA(OFF, BASE, IMM, TAG) asm volatile("global_load_lds_dwordx4 %0, %1 offset:" #IMM " ; @dma %2" ::"v"(OFF), "s"(BASE), "n"(TAG) : "memory")
  auto dma = [&](int u, int buf, auto tagc) {  // the tile this DMA fetches is t + tagc
    constexpr int TAG = decltype(tagc)::value;
    const bool isa = u < GA;
    const int q = isa ? u : u - GA;
    if (q % 4 == 0) {
      const unsigned m0v = (isa ? lds_a : lds_b) + buf * IMG * 8 + (q / 4) * 4096;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" ::"s"(m0v) : "memory");
    }
    const unsigned off = isa ? oa[q] : ob[q];
    const char* base = isa ? sa : sb;
    if (q % 4 == 0) KW_DMA(off, base, 0, TAG);
    if (q % 4 == 1) KW_DMA(off, base, 1024, TAG);
    if (q % 4 == 2) KW_DMA(off, base, 2048, TAG);
    if (q % 4 == 3) KW_DMA(off, base, 3072, TAG);
  };
#undef KW_DMA

  // Fragment reads (round 4, as gemm_kwave.hip): a read's address = one per-lane base for (operand, half-tile), + the image's
  // offset (one add per half), + a constant per read in the instruction's offset field -- no address arithmetic per read;
  // two sets of landing registers, one per half-tile parity, and the MFMAs take their operands straight from the set the
  // reads landed in -- no unpacking moves (the loop carried ~80 VALU instructions per k-tile next to its 64 MFMAs).
  // (reads land in registers whose first consumer is the wait: see gemm_kwave.hip)
  f64x2 ta[2][RA], tb[2][RB];
  unsigned a_lane[2], b_lane[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    a_lane[h] = lds_a + (AMODE == 1 ? ((8 * h + 2 * kg) * BM + TM * l15) * 8 : (l15 * BK + 2 * ((4 * h + kg) ^ (l15 & 7))) * 8);
    b_lane[h] = lds_b + (BMODE == 0 ? ((8 * h + 2 * kg) * BN + TN * l15) * 8 : (l15 * BK + 2 * ((4 * h + kg) ^ (l15 & 7))) * 8);
  }
  auto rd = [](f64x2& dst, unsigned addr, auto off, auto tagc) {
    asm volatile("ds_read_b128 %0, %1 offset:%2 ; @rd %3" : "=v"(dst) : "v"(addr), "n"(decltype(off)::value), "n"(decltype(tagc)::value));
  };
  // read r of the half whose lane bases (+ image offset) are abase / bbase, into set `slot`; tagc: the image of tile t + tagc
  auto frag = [&](int slot, unsigned abase, unsigned bbase, auto ri, auto tagc) {
    constexpr int r = decltype(ri)::value;
    if constexpr (r < RA) {
      // owning (m-contiguous): r = (k-step e of the half, row pair q): rows TM l15 + 2q, +1; k-contiguous: r = tile, row 16 r + l15
      constexpr int off = AMODE == 1 ? ((r / (TM / 2)) * BM + 2 * (r % (TM / 2))) * 8 : r * 16 * BK * 8;
      rd(ta[slot][r], abase, std::integral_constant<int, off>{}, tagc);
    } else {
      constexpr int rr = r - RA;
      constexpr int off = BMODE == 0 ? ((rr / (TN / 2)) * BN + 2 * (rr % (TN / 2))) * 8 : rr * 16 * BK * 8;
      rd(tb[slot][rr], bbase, std::integral_constant<int, off>{}, tagc);
    }
  };
  // the reads issued since the last landing are complete: set `slot` is valid from here on
  auto land = [&](int slot) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ta[slot][0]), "+v"(ta[slot][1]), "+v"(ta[slot][2]), "+v"(ta[slot][3])::"memory");
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tb[slot][0]), "+v"(tb[slot][1]), "+v"(tb[slot][2]), "+v"(tb[slot][3])::"memory");
  };

#define KW64_PIN_ACC asm volatile("" : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[1][0]), "+a"(acc[1][1]), \
    "+a"(acc[1][2]), "+a"(acc[1][3]), "+a"(acc[2][0]), "+a"(acc[2][1]), "+a"(acc[2][2]), "+a"(acc[2][3]), "+a"(acc[3][0]), "+a"(acc[3][1]), \
    "+a"(acc[3][2]), "+a"(acc[3][3]))
  auto tile = [&](auto dma_on, int buf, int bnext) {
    constexpr bool DMA = decltype(dma_on)::value;
    kw64_static_for<0, 2>([&](auto hi) {
      constexpr int h = decltype(hi)::value, cur = h, nxt = h ^ 1;
      if constexpr (h == 1) {
        if constexpr (DMA) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NI - 2) * (GA + GB)) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_sched_barrier(0);
      // (the reads of this half fetch the NEXT half: image buf, second half -- or the next tile's image, first half)
      const unsigned abase = a_lane[h ^ 1] + (h == 0 ? buf : bnext) * IMG * 8, bbase = b_lane[h ^ 1] + (h == 0 ? buf : bnext) * IMG * 8;
      kw64_static_for<0, 2 * TM * TN>([&](auto ni) {
        constexpr int n = decltype(ni)::value;
        constexpr int e = n / (TM * TN), i = (n % (TM * TN)) / TN, jn = n % TN;
        double av, bv;
        if constexpr (AMODE == 1) av = ta[cur][e * (TM / 2) + i / 2][i % 2]; else av = ta[cur][i][e];
        if constexpr (BMODE == 0) bv = tb[cur][e * (TN / 2) + jn / 2][jn % 2]; else bv = tb[cur][jn][e];
        // (inline asm with the accumulator pinned to AccVGPRs: with the builtin the compiler carried the 128 accumulator
        // registers across the loop's back edge in VGPRs and moved them into AccVGPRs and back out every k-tile -- 256
        // moves next to 64 MFMAs)
        asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+a"(acc[i][jn]) : "v"(av), "v"(bv));
        if constexpr (n < RA + RB) {
          frag(nxt, abase, bbase, ni, std::integral_constant<int, h>{});   // (h == 0: this tile's image, h == 1: the next tile's)
        } else if constexpr (DMA && h == 1 && n < RA + RB + GA + GB) {
          dma(n - (RA + RB), buf, std::integral_constant<int, NI>{});
          if constexpr (n == RA + RB + GA + GB - 1) {
            sa += step_a;
            sb += step_b;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      });
      land(nxt);
      __builtin_amdgcn_sched_barrier(0);
    });
    asm volatile("; @advance");   // (for the checker: the loop's t becomes t + 1)
    // (the accumulators cross the loop's back edge IN AccVGPRs: without this the register allocator carried half of them
    // in VGPRs for two of the four operand layouts and copied them in and out around the MFMAs of every k-tile)
    KW64_PIN_ACC;
  };

  KW64_PIN_ACC;
  if (nT > 0) {
    asm volatile("; @images %0 private" ::"n"(NI));
    // (two written-out paths, each with the wait that matches what it issued: the hazard checker is not path-sensitive)
    static_assert(NI == 2, "the prologue is written out for two images");
    if (nT >= NI) {
#pragma unroll
      for (int u = 0; u < GA + GB; ++u) dma(u, 0, std::integral_constant<int, 0>{});
      sa += step_a;
      sb += step_b;
#pragma unroll
      for (int u = 0; u < GA + GB; ++u) dma(u, 1, std::integral_constant<int, 1>{});
      sa += step_a;
      sb += step_b;
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NI - 1) * (GA + GB)) : "memory");
    } else {
#pragma unroll
      for (int u = 0; u < GA + GB; ++u) dma(u, 0, std::integral_constant<int, 0>{});
      sa += step_a;
      sb += step_b;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    kw64_static_for<0, RA + RB>([&](auto ri) { frag(0, a_lane[0], b_lane[0], ri, std::integral_constant<int, 0>{}); });
    land(0);
    __builtin_amdgcn_sched_barrier(0);
    int buf = 0, t = 0;
    for (; t + NI < nT; ++t) {
      const int bnext = buf + 1 == NI ? 0 : buf + 1;
      tile(std::true_type{}, buf, bnext);
      buf = bnext;
    }
    for (; t < nT; ++t) {
      const int bnext = buf + 1 == NI ? 0 : buf + 1;
      tile(std::false_type{}, buf, bnext);
      buf = bnext;
    }
  }
  // The last MFMAs retire before anything but another MFMA touches the AccVGPRs: the accumulators are read-write operands
  // of the statement that holds the wait states (the compiler pads the hazards of the MFMAs it issues itself, not those of
  // an asm string; tools/asm_inflight_check.py rule 6; gemm_kwave.hip).
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15"
               : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[1][0]), "+a"(acc[1][1]), "+a"(acc[1][2]),
                 "+a"(acc[1][3]), "+a"(acc[2][0]), "+a"(acc[2][1]), "+a"(acc[2][2]), "+a"(acc[2][3]), "+a"(acc[3][0]), "+a"(acc[3][1]),
                 "+a"(acc[3][2]), "+a"(acc[3][3])::"memory");

  // the ragged end of K (fewer than 16): the last wave, operands straight from global memory, four k per MFMA
  if (g.K % BK != 0 && wave == NW - 1) {
    long ra[TM], cb[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      long m = m0 + (AMODE == 1 ? TM * l15 + i : i * 16 + l15);
      ra[i] = (m < g.M ? m : g.M - 1) * g.a_sm;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      long n = n0 + (BMODE == 0 ? TN * l15 + j : j * 16 + l15);
      cb[j] = (n < g.N ? n : g.N - 1) * g.b_sn;
    }
    for (int kk = KT * BK; kk < g.K; kk += 4) {
      const int k = kk + kg;
      const bool ok = k < g.K;
      const long kc = ok ? k : g.K - 1;
      double av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const double v = g.A[ra[i] + kc * g.a_sk];
        av[i] = ok ? v : 0.0;
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const double v = g.B[kc * g.b_sk + cb[j]];
        bv[j] = ok ? v : 0.0;
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
  }

  // partial tiles -> LDS (each wave into its own, now dead, images), summed in wave order
  // D reg r lane l -> row (l>>4) + 4 r, col l&15 of the MFMA tile
  {
    double* P = smem + wave * WAVE_DOUBLES;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = BMODE == 0 ? TN * l15 + j : j * 16 + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int tr = kg + 4 * r;
          const int row = AMODE == 1 ? TM * tr + i : i * 16 + tr;
          P[row * BN + col] = acc[i][j][r];
        }
      }
  }
  __syncthreads();
  // (two instantiations of the way out: a plain product has no per-element branches on bias / activation / act')
  auto finish = [&](auto plainc) {
    constexpr bool PLAIN = decltype(plainc)::value;
    for (int q = tid; q < BM * BN / 2; q += NW * 64) {
      const int row = q / (BN / 2), c2 = (q % (BN / 2)) * 2;
      f64x2 s = *reinterpret_cast<const f64x2*>(smem + row * BN + c2);
#pragma unroll
      for (int w = 1; w < NW; ++w) s += *reinterpret_cast<const f64x2*>(smem + w * WAVE_DOUBLES + row * BN + c2);
      const long gr = m0 + row, gc = n0 + c2;
      if (gr >= g.M || gc >= g.N) continue;
      double* dst = g.C + gr * g.c_sm + gc;
      if constexpr (PLAIN) {  // (wide: N % 2 == 0, a pair is in or out)
        *reinterpret_cast<f64x2*>(dst) = g.alpha * s;
      } else {
        double v[2] = {s.x, s.y};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          if (gc + e >= g.N) break;
          double x = g.alpha * v[e];
          if (g.cin) x += g.beta * g.cin[gr * g.c_sm + gc + e];
          if (g.bias) x += g.bias[gc + e];
          if (g.act == 1) x = dm::logistic(x);
          else if (g.act == 2) x = tanh(x);
          if (g.dact) {
            const double hh = g.dact[gr * g.c_sm + gc + e];
            x *= g.dact_kind ? 1.0 - hh * hh : hh * (1.0 - hh);
          }
          v[e] = x;
        }
        if (g.wide) {
          f64x2 o = {v[0], v[1]};
          *reinterpret_cast<f64x2*>(dst) = o;
        } else {
#pragma unroll
          for (int e = 0; e < 2; ++e)
            if (gc + e < g.N) dst[e] = v[e];
        }
      }
    }
  };
  if (g.wide && !g.bias && g.act == 0 && !g.dact && !g.cin) finish(std::true_type{});
  else finish(std::false_type{});
}

static int kw64_mode() {
  static const int m = [] { const char* e = ab_getenv("TOPS_GEMM64_KW"); return e ? atoi(e) : 1; }();
  return m;
}

static bool kw64_can(const GemmProblem& p) {
  if (p.dtype != TO_F64 || p.batch != 1 || p.reduce_batch || p.rowsum || p.loss_rows || (p.beta != 0.0 && !p.Cin)) return false;
  if (p.M < 16 || p.N < 16 || (p.M < 128 && p.N < 128) || p.K < 16) return false;   // (16 .. 127 rows or columns: the last tile is padding; loads clamp, stores are guarded)
  if (p.M > 2147483647LL || p.N > 2147483647LL || p.K > 2147483647LL) return false;
  const bool a_k = p.a_sk == 1, a_m = !a_k && p.a_sm == 1;
  const bool b_n = p.b_sn == 1, b_k = !b_n && p.b_sk == 1;
  if (!(a_k || a_m) || !(b_n || b_k)) return false;
  auto al8 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7u) == 0; };
  if (!al8(p.A) || !al8(p.B)) return false;
  const int64_t ext_a = a_k ? p.M * p.a_sm : 16 * p.a_sk + p.M, ext_b = b_k ? p.N * p.b_sn : 16 * p.b_sk + p.N;
  if (ext_a * 8 + 8192 >= (1LL << 32) || ext_b * 8 + 8192 >= (1LL << 32) || p.a_sm < 0 || p.a_sk < 0 || p.b_sk < 0 || p.b_sn < 0) return false;
  if (a_m && p.M % 2 != 0) return false;  // an m-contiguous pair must be in or out of the matrix as a whole
  if (b_n && p.N % 2 != 0) return false;
  return true;
}

bool gemm_kw64_applicable(const GemmProblem& p) {
  const int mode = kw64_mode();
  if (mode == 0 || !kw64_can(p)) return false;
  if (mode >= 2) return true;
  // 128 KiB of LDS and ~330 registers: one workgroup per CU, so the win is where ONE round of 64x64 tiles covers the
  // output (ours before / now, TF: 768^3 16 / 25, 1000^3 20 / 44, 1024^3 25 / 43, 4096 x 784 x 256 26 / 43); from two
  // rounds on the tiled kernel is ahead again (1536^3 50 / 37, 2048^3 63 / 52)
  const long t64 = ((p.M + 63) / 64) * ((p.N + 63) / 64);
  if (t64 >= 100 && t64 <= 320 && p.K >= 128) return true;
  // Round 6 (last), tools/gemm_scan.py with SCAN_DTYPE=f64 (profiles/r06_gemm_scan_f64_*.txt): 432 of 969 shapes below 0.92 of the
  // vendor fp64 GEMM, half of them at 0.5 -- every extent the 256x128 tiles do not fit went to the compiler-scheduled kernel
  // (~23 TF).  This kernel forced onto those rows was 1.2 .. 2.6 x ahead on 181 of the 302 without a sliver (us, before / here;
  // vendor): 256 x 10000 x 10000 2180 / 848 (1089), 784 x 4096 x 2048 489 / 236 (245), 300 x 4096 x 60000 5070 / 2289 (3113),
  // 60000 x 784 x 300 803 / 519 (556), 2048 x 300 x 1024 97 / 28 (24); and on shapes the tiles DO fit up to 1,024 tiles
  // (2048 x 1024 x 1024 89 / 67 (73), 2048 x 256 x 1024 57 / 24 (20)); behind from a few thousand tiles on where they fit
  // (2048 x 256 x 60000 1045 / 1367).
  if (t64 < 100 || p.K < 64) return false;
  const long narrow = p.M < p.N ? p.M : p.N;
  if (narrow < 128 && t64 < 200) return false;   // (100 x 4096 x 4096: 97 us on the small-GEMM route, 118 here; 10000 x K x 100 twice as fast here)
  // (K <= 256 under thousands of tiles with both extents large: block + strips on the tiled kernel is ahead -- 2048 x 256 x 60000
  //  1.04 ms there, 1.36 here; 784 x 256 x 60000 0.62 / 0.54 the other way)
  if (p.K <= 256 && p.K % 16 == 0 && narrow >= 1024 && t64 > 2048) return false;
  const bool fits = p.M % 256 == 0 && p.N % 128 == 0 && p.K % 16 == 0;
  return !fits || t64 <= 1024;
}

// A tile per WAVE (the fp32 kernel's SPLIT = false): a K of a few hundred is not worth sharing among four waves.
static bool kw64_wave_per_tile(const GemmProblem& p) {
  static const int forced = [] { const char* e = ab_getenv("TOPS_GEMM64_KW_NW"); return e ? atoi(e) : 0; }();   // (development: 1 / 4)
  if (forced) return forced == 1;
  const long t64 = ((p.M + 63) / 64) * ((p.N + 63) / 64);
  // us, four waves a tile / a wave a tile: 4096 x 100 x 4096 121 / 101, 60000 x 100 x 1024 480 / 335, 2048 x 100 x 2048 33 / 21; behind from
  // K = 256 on (4096 x 256 x 4096 179 / 212, 10000 x 784 x 2048 537 / 710: one wave a SIMD has nothing to hide its waits under)
  // (... and two waves a tile are ahead of both from two tiles a CU on: 4096 x 100 x 4096 121 / 102 / 88, 4096 x 128 x 4096 122 / 120 / 96)
  return t64 >= 1024 && t64 < 2048 && p.K <= 128;
}

void launch_gemm_kw64(const GemmProblem& p, hipStream_t s) {
  Kw64Args g{};
  g.A = (const double*)p.A; g.B = (const double*)p.B; g.C = (double*)p.C;
  g.M = (int)p.M; g.N = (int)p.N; g.K = (int)p.K;
  g.a_sm = p.a_sm; g.a_sk = p.a_sk; g.b_sk = p.b_sk; g.b_sn = p.b_sn; g.c_sm = p.c_sm;
  g.tiles_m = (int)((p.M + 63) / 64);
  g.tiles_n = (int)((p.N + 63) / 64);
  g.alpha = p.alpha;
  g.bias = (const double*)p.bias; g.dact = (const double*)p.dact; g.act = p.act; g.dact_kind = p.dact_kind;
  g.cin = p.beta != 0.0 ? (const double*)p.Cin : nullptr; g.beta = (double)p.beta;
  g.wide = (reinterpret_cast<uintptr_t>(p.C) & 15u) == 0 && p.c_sm % 2 == 0 && p.N % 2 == 0;
  const int mode = (p.a_sk == 1 ? 0 : 2) + (p.b_sn == 1 ? 0 : 1);
  dim3 grid(g.tiles_m * g.tiles_n);
  // Two waves a tile (64 KiB of LDS: two workgroups a CU) from two tiles a CU on: the K loop is shared by two waves instead of four
  // and a CU works on two tiles at once -- us, four / two waves: 4096 x 256 x 4096 177 / 152, 10000 x 784 x 2048 536 / 486,
  // 2048 x 2048 x 2048 247 / 239; at one tile a CU half the SIMDs would idle (1024^3 34.5 / 62.2).
  static const int nw_forced = [] { const char* e = ab_getenv("TOPS_GEMM64_KW_NW"); return e ? atoi(e) : 0; }();
  const long t64 = (long)g.tiles_m * g.tiles_n;
  if (nw_forced == 2 || (nw_forced == 0 && t64 >= 512 && !kw64_wave_per_tile(p))) {
    const dim3 block(128);
    switch (mode) {
      case 0: launch_k((gemm_kw64_kernel<0, 0, 2, 2>), grid, block, 0, s, g); break;
      case 1: launch_k((gemm_kw64_kernel<0, 1, 2, 2>), grid, block, 0, s, g); break;
      case 2: launch_k((gemm_kw64_kernel<1, 0, 2, 2>), grid, block, 0, s, g); break;
      default: launch_k((gemm_kw64_kernel<1, 1, 2, 2>), grid, block, 0, s, g); break;
    }
    TO_HIP(hipGetLastError());
    count_launch();
    return;
  }
  if (kw64_wave_per_tile(p)) {   // (NW = 1: a workgroup IS a wave -- 32 KiB of LDS, four or five of them a CU)
    const dim3 block(64);
    switch (mode) {
      case 0: launch_k((gemm_kw64_kernel<0, 0, 1, 2>), grid, block, 0, s, g); break;
      case 1: launch_k((gemm_kw64_kernel<0, 1, 1, 2>), grid, block, 0, s, g); break;
      case 2: launch_k((gemm_kw64_kernel<1, 0, 1, 2>), grid, block, 0, s, g); break;
      default: launch_k((gemm_kw64_kernel<1, 1, 1, 2>), grid, block, 0, s, g); break;
    }
  } else {
    const dim3 block(256);
    switch (mode) {
      case 0: launch_k((gemm_kw64_kernel<0, 0, 4, 2>), grid, block, 0, s, g); break;
      case 1: launch_k((gemm_kw64_kernel<0, 1, 4, 2>), grid, block, 0, s, g); break;
      case 2: launch_k((gemm_kw64_kernel<1, 0, 4, 2>), grid, block, 0, s, g); break;
      default: launch_k((gemm_kw64_kernel<1, 1, 4, 2>), grid, block, 0, s, g); break;
    }
  }
  TO_HIP(hipGetLastError());
  count_launch();
}

// ---- the fp64 tile MENU: 48x48 / 48x64 / 64x48 / 32x64 / 64x32 ---------------------------------------------------------------
// A few hundred 64x64 tiles quantise badly against 256 CUs (768^3: 144 tiles -- and exactly 256 of 48x48; 1024 x 512 x 1024:
// 128 tiles -- and 256 of 64x32).  gemm_kw64_menu_kernel is gemm_kw16.hip's answer on v_mfma_f64_16x16x4_f64 blocks: an output
// tile of TM x TN blocks, one workgroup of four waves a tile, the K loop split over the waves, every wave DMA-feeding its own
// LDS images and waiting on nothing but its own vmcnt, no barrier in the loop, the four partial tiles summed in LDS in wave
// order, XCD-aware tile order, accumulators in AccVGPRs.  Off unless to_set_gemm_f64_menu turns it on.
//
// Fragments.  A k-tile (16 k) is 4 TM TN MFMAs in four steps s = (h, e); the lanes of k-group kg use k = 8 h + 2 kg + e in
// step s, A and B alike.
//  - k-contiguous operand, image [x][8 chunks of 2 k] (a row is 128 B), chunk c of row x in slot c ^ ((x >> 1) & 7): a lane's
//    fragment of a block and a half h is ONE ds_read_b128 (chunk 4 h + kg: both e).  The sixteen lanes a ds_read_b128 serves
//    together (one kg, x = 0 .. 15) sit at byte x * 128 + slot * 16: bank group (x & 1) * 8 + slot, and (x & 1, (x >> 1) & 7)
//    takes sixteen values -- the 64 banks once.  (gemm_kw64_kernel's c ^ (x & 7) puts x and x + 8 on the same banks.)  Block r
//    is rows 16 r + x: + 2 KiB, the swizzle unchanged, so any multiple of 16 rows is an image.
//  - m-/n-contiguous operand, image [rho(k)][rows], rho(k) = 8 h + 4 e + kg: ROW PAIRS.  "Lane l15 owns rows TM l15 .." needs
//    16-byte alignment of TM doubles, i.e. TM even, and 64 = 16 * 4 rows; here a lane owns the PAIR 2 l15, 2 l15 + 1 of every
//    32 rows (one ds_read_b128 per step: blocks 2 p and 2 p + 1 of pair-group p hold rows 32 p + 2 x + {0, 1}) and, where TM
//    is odd, row 32 P + l15 of the last sixteen (one ds_read_b64: block 2 P in the plain order).  The sixteen lanes of a
//    b128 read 256 contiguous bytes: the banks once, whatever the pitch (384 B at 48 rows).  The thirty-two lanes of a b64
//    are k-groups kg, kg + 1: image rows rho, rho + 1 -- with a 384-byte pitch the two 128-byte runs sit in different halves
//    of the 256 bytes of banks (the plain [k] order would put k and k + 2 on the same half: that is what rho is for).
//    The epilogue maps block rows back (row_of below).
// LDS and NI.  A wave's images are NI (BM + BN) 16 * 8 B: 24 KiB at 48x48 and 32x64, 28 KiB at 48x64 with NI = 2 (96 / 112 KiB
// a workgroup of the 160); its partial tile (18 / 16 / 24 KiB) fits them once they are dead.  NI = 3 would fit 48x48 and 32x64
// (144 KiB) but not 48x64 (168 KiB), and no tile gets a second workgroup on the CU either way.  It is not needed: an fp64
// 16x16x4 MFMA occupies the matrix pipe 64 cycles (32 flop / clk / SIMD), twice the fp32 one, so ONE k-tile is 2,048 (32x64)
// .. 3,072 (48x64) cycles of MFMA time -- what gemm_kw16.hip buys with two (1,152 each at 48x48) -- provided the DMA has the
// whole tile to land.  So the order inside a tile differs from both siblings: the fetch of tile t + 2 goes FIRST (into the
// image tile t's fragments were read from during tile t - 1), behind the first GA + GB MFMAs; then the wait for tile t + 1
// (vmcnt(GA + GB): everything but what this tile just issued), which had all of tile t - 1 and these MFMAs to land; then tile
// t + 1's fragments into the other register set.  80-wide tiles: 80x80 needs 2 * 160 * 128 B = 40 KiB a wave, 160 KiB a
// workgroup -- all of it, none left for alignment -- with a 50 KiB partial tile that does not fit the 40; 64x80 is 36 KiB a wave
// = 144 KiB and a 40 KiB partial tile: does not fit either.  Not built.
// Registers: 8 AccVGPRs a block: 72 (3x3), 96 (3x4), 64 (2x4); two sets of fragments, at most 2 * (32 + 32) VGPRs.
// A K that is no multiple of 16: as gemm_kw64_kernel, the last wave adds the ragged k-tile straight from global memory.
// Odd runs, short runs: gemm_kw16.hip's ghost tile and always-fetch (one loop body, one wait count).
struct Kw64mShape { int tm, tn; };
static const Kw64mShape kw64m_menu[] = {{3, 3}, {3, 4}, {4, 3}, {2, 4}, {4, 2}};
constexpr int KW64M_TILES = (int)(sizeof(kw64m_menu) / sizeof(kw64m_menu[0]));

// row (column) of the tile that block b's index x (0 .. 15) stands for; PAIRED: the operand is m-/n-contiguous
template <bool PAIRED, int T>
__device__ __forceinline__ constexpr int kw64m_row_of(int b, int x) {
  if (!PAIRED || b >= 2 * (T / 2)) return 16 * b + x;
  return 32 * (b / 2) + 2 * x + (b % 2);
}

template <int AMODE, int BMODE, int TM, int TN>
__global__ __launch_bounds__(256) void gemm_kw64_menu_kernel(Kw64Args g) {
  constexpr int NW = 4, NI = 2, BM = 16 * TM, BN = 16 * TN, BK = 16, GA = BM / 8, GB = BN / 8;   // GA / GB: 1-KiB DMA pieces per image
  constexpr int IMG_A = BM * BK, IMG_B = BN * BK;       // doubles per image
  constexpr int WAVE_DOUBLES = NI * (IMG_A + IMG_B);    // a wave's LDS: [NI] A images, [NI] B images
  constexpr bool PA = AMODE == 1, PB = BMODE == 0;      // paired (m-/n-contiguous) operands
  constexpr int PAIRS_A = TM / 2, ODD_A = TM % 2, PAIRS_B = TN / 2, ODD_B = TN % 2;
  static_assert(BM * BN <= WAVE_DOUBLES, "the partial tile fits the wave's (dead) images");
  static_assert(NW * WAVE_DOUBLES * 8 <= 160 * 1024, "a workgroup's LDS");
  static_assert(GA <= 8 && GB <= 8, "piece offsets are written out up to 8 KiB");
  __shared__ __attribute__((aligned(16))) double smem[NW * WAVE_DOUBLES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, kg = lane >> 4;
  // XCD-aware tile order (as gemm_kw64_kernel)
  const int ntiles = g.tiles_m * g.tiles_n;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = ntiles >> 3, r = ntiles & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  int tile_m, tile_n;
  {
    constexpr int R = 4;
    const int band = bid / (R * g.tiles_n);
    const int rows = (g.tiles_m - band * R) < R ? (g.tiles_m - band * R) : R;
    const int in = bid - band * R * g.tiles_n;
    tile_n = in / rows;
    tile_m = band * R + in % rows;
  }
  const long m0 = (long)tile_m * BM, n0 = (long)tile_n * BN;

  f64x4 acc[TM * TN];
#pragma unroll
  for (int i = 0; i < TM * TN; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int KT = g.K / BK;
  const int per = 2 * ((KT + 2 * NW - 1) / (2 * NW));   // (even runs: the K loop is written out two k-tiles at a time)
  const int t_begin = wave * per < KT ? wave * per : KT;
  const int t_end = t_begin + per < KT ? t_begin + per : KT;
  const int nT = t_end - t_begin;

  typedef __attribute__((address_space(3))) void* lptr_t;
  const unsigned lds_a = (unsigned)(unsigned long)(lptr_t)(smem + wave * WAVE_DOUBLES);  // [NI][IMG_A]
  const unsigned lds_b = lds_a + NI * IMG_A * 8;                                         // [NI][IMG_B]

  // LDS reads per k-tile: k-contiguous 2 a block (the halves); paired 4 steps x (pairs + the odd block)
  constexpr int RA = PA ? 4 * (PAIRS_A + ODD_A) : 2 * TM, RB = PB ? 4 * (PAIRS_B + ODD_B) : 2 * TN;
  static_assert(RA + RB + GA + GB <= 4 * TM * TN, "a slot behind every MFMA");
  // DMA: a piece is 1 KiB = 128 doubles of the image, lane l fills doubles 128 q + 2 l, + 1; scalar base + per-lane 32-bit
  // byte offset, piece q's offset biased by -(q % 4) KiB, the base by -3 KiB (gemm_kwave.hip)
  unsigned oa[GA], ob[GB];
#pragma unroll
  for (int q = 0; q < GA; ++q) {
    const int f = q * 128 + lane * 2;
    long e;
    if constexpr (PA) {
      const int kr = f / BM;   // image row rho -> k = 8 h + 2 kg + e of rho = 8 h + 4 e + kg
      long m = m0 + f % BM;    // two consecutive rows (M even: a pair is in or out)
      if (m + 2 > g.M) m = g.M - 2;
      e = (long)(8 * (kr >> 3) + 2 * (kr & 3) + ((kr >> 2) & 1)) * g.a_sk + m;
    } else {
      const int x = f / BK;
      long m = m0 + x;
      if (m >= g.M) m = g.M - 1;
      e = m * g.a_sm + 2 * (((f % BK) / 2) ^ ((x >> 1) & 7));
    }
    oa[q] = (unsigned)(e * 8 + 3072 - (q % 4) * 1024);
  }
#pragma unroll
  for (int q = 0; q < GB; ++q) {
    const int f = q * 128 + lane * 2;
    long e;
    if constexpr (PB) {
      const int kr = f / BN;
      long n = n0 + f % BN;
      if (n + 2 > g.N) n = g.N - 2;
      e = (long)(8 * (kr >> 3) + 2 * (kr & 3) + ((kr >> 2) & 1)) * g.b_sk + n;
    } else {
      const int x = f / BK;
      long n = n0 + x;
      if (n >= g.N) n = g.N - 1;
      e = n * g.b_sn + 2 * (((f % BK) / 2) ^ ((x >> 1) & 7));
    }
    ob[q] = (unsigned)(e * 8 + 3072 - (q % 4) * 1024);
  }
  const long step_a = (PA ? (long)BK * g.a_sk : BK) * 8, step_b = (PB ? (long)BK * g.b_sk : BK) * 8;  // bytes
  const char* sa = reinterpret_cast<const char*>(g.A) - 3072 + (long)t_begin * step_a;
  const char* sb = reinterpret_cast<const char*>(g.B) - 3072 + (long)t_begin * step_b;
  // (`; @dma K` / `; @rd K` / `; @images` / `; @advance`: which k-tile's image, relative to the loop's current tile t, an
  //  access touches -- comments for tools/asm_inflight_check.py, see gemm_kwave.hip)
#define KWM_DMA(OFF, BASE, IMM, TAG) asm volatile("global_load_lds_dwordx4 %0, %1 offset:" #IMM " ; @dma %2" ::"v"(OFF), "s"(BASE), "n"(TAG) : "memory")
  auto dma = [&](int u, int buf, auto tagc) {  // the tile this DMA fetches is t + tagc
    constexpr int TAG = decltype(tagc)::value;
    const bool isa = u < GA;
    const int q = isa ? u : u - GA;
    if (q % 4 == 0) {
      const unsigned m0v = (isa ? lds_a + buf * IMG_A * 8 : lds_b + buf * IMG_B * 8) + (q / 4) * 4096;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" ::"s"(m0v) : "memory");
    }
    const unsigned off = isa ? oa[q] : ob[q];
    const char* base = isa ? sa : sb;
    if (q % 4 == 0) KWM_DMA(off, base, 0, TAG);
    if (q % 4 == 1) KWM_DMA(off, base, 1024, TAG);
    if (q % 4 == 2) KWM_DMA(off, base, 2048, TAG);
    if (q % 4 == 3) KWM_DMA(off, base, 3072, TAG);
  };
#undef KWM_DMA

  // Fragment reads: an address = one of two per-lane bases of the operand (k-contiguous: the halves, whose slots differ by
  // an XOR; paired: the pairs and the odd block) + the image's offset + a constant in the instruction's offset field.  Two
  // sets of landing registers, one per tile parity; their first consumer is the wait (gemm_kwave.hip has the story).
  f64x2 ta2[2][PA ? (4 * PAIRS_A > 0 ? 4 * PAIRS_A : 1) : 2 * TM], tb2[2][PB ? (4 * PAIRS_B > 0 ? 4 * PAIRS_B : 1) : 2 * TN];
  double ta1[2][PA && ODD_A ? 4 : 1], tb1[2][PB && ODD_B ? 4 : 1];   // the odd block of a paired operand: [step]
  unsigned a_lane[2], b_lane[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    a_lane[h] = lds_a + (PA ? (kg * BM + (h == 0 ? 2 * l15 : 32 * PAIRS_A + l15)) * 8 : (l15 * BK + 2 * ((4 * h + kg) ^ ((l15 >> 1) & 7))) * 8);
    b_lane[h] = lds_b + (PB ? (kg * BN + (h == 0 ? 2 * l15 : 32 * PAIRS_B + l15)) * 8 : (l15 * BK + 2 * ((4 * h + kg) ^ ((l15 >> 1) & 7))) * 8);
  }
  auto rd2 = [](f64x2& dst, unsigned addr, auto off, auto tagc) {
    asm volatile("ds_read_b128 %0, %1 offset:%2 ; @rd %3" : "=v"(dst) : "v"(addr), "n"(decltype(off)::value), "n"(decltype(tagc)::value));
  };
  auto rd1 = [](double& dst, unsigned addr, auto off, auto tagc) {
    asm volatile("ds_read_b64 %0, %1 offset:%2 ; @rd %3" : "=v"(dst) : "v"(addr), "n"(decltype(off)::value), "n"(decltype(tagc)::value));
  };
  // read r of a k-tile's fragments (image byte offsets aimg / bimg), into set `slot`
  auto frag = [&](int slot, unsigned aimg, unsigned bimg, auto ri, auto tagc) {
    constexpr int r = decltype(ri)::value;
    if constexpr (r < RA) {
      if constexpr (!PA) {          // r = (block, half)
        rd2(ta2[slot][r], a_lane[r % 2] + aimg, std::integral_constant<int, (r / 2) * 16 * BK * 8>{}, tagc);
      } else {                      // r = (step s, u): image row 8 h + 4 e (+ kg in the base) = 4 s'; u < pairs: pair-group u, else the odd block
        constexpr int s = r / (PAIRS_A + ODD_A), u = r % (PAIRS_A + ODD_A), krow = 8 * (s / 2) + 4 * (s % 2);
        if constexpr (u < PAIRS_A) rd2(ta2[slot][s * PAIRS_A + u], a_lane[0] + aimg, std::integral_constant<int, (krow * BM + 32 * u) * 8>{}, tagc);
        else rd1(ta1[slot][s], a_lane[1] + aimg, std::integral_constant<int, krow * BM * 8>{}, tagc);
      }
    } else {
      constexpr int rr = r - RA;
      if constexpr (!PB) {
        rd2(tb2[slot][rr], b_lane[rr % 2] + bimg, std::integral_constant<int, (rr / 2) * 16 * BK * 8>{}, tagc);
      } else {
        constexpr int s = rr / (PAIRS_B + ODD_B), u = rr % (PAIRS_B + ODD_B), krow = 8 * (s / 2) + 4 * (s % 2);
        if constexpr (u < PAIRS_B) rd2(tb2[slot][s * PAIRS_B + u], b_lane[0] + bimg, std::integral_constant<int, (krow * BN + 32 * u) * 8>{}, tagc);
        else rd1(tb1[slot][s], b_lane[1] + bimg, std::integral_constant<int, krow * BN * 8>{}, tagc);
      }
    }
  };
  // the reads issued since the last landing are complete: set `slot` is valid from here on (every register of the set is an
  // operand of a wait, so whatever the compiler does with it, it does behind the wait)
  auto land = [&](int slot) {
#pragma unroll
    for (int i = 0; i < (int)(sizeof(ta2[0]) / sizeof(f64x2)); ++i) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ta2[slot][i])::"memory");
#pragma unroll
    for (int i = 0; i < (int)(sizeof(tb2[0]) / sizeof(f64x2)); ++i) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tb2[slot][i])::"memory");
    if constexpr (PA && ODD_A) {
#pragma unroll
      for (int i = 0; i < 4; ++i) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ta1[slot][i])::"memory");
    }
    if constexpr (PB && ODD_B) {
#pragma unroll
      for (int i = 0; i < 4; ++i) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tb1[slot][i])::"memory");
    }
  };
  auto zero = [&](int slot) {   // a ghost tile's fragments
#pragma unroll
    for (int i = 0; i < (int)(sizeof(ta2[0]) / sizeof(f64x2)); ++i) ta2[slot][i] = f64x2{0.0, 0.0};
#pragma unroll
    for (int i = 0; i < (int)(sizeof(tb2[0]) / sizeof(f64x2)); ++i) tb2[slot][i] = f64x2{0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (PA && ODD_A) ta1[slot][i] = 0.0;
      if constexpr (PB && ODD_B) tb1[slot][i] = 0.0;
    }
  };

  // one k-tile: 4 TM TN MFMAs, behind each one pinned other instruction: FIRST the fetch of tile t + NI into the image this
  // tile's fragments came from (they landed at the end of the previous tile), then -- behind the wait that leaves only those
  // fetches in flight -- the next tile's fragments into the other set.  EVERY tile fetches: where tile t + NI does not exist
  // the wave's last tile is fetched again into an image nobody reads (one body, one wait count: gemm_kw16.hip).
  // an asm statement with every accumulator as a "+a" operand: the drain's wait states, and -- empty -- what keeps the
  // accumulators in AccVGPRs across the loop's edges (gemm_kw64_kernel's KW64_PIN_ACC; tools/asm_acc_lint.py)
#define KWM_ACC8 "+a"(acc[0]), "+a"(acc[1]), "+a"(acc[2]), "+a"(acc[3]), "+a"(acc[4]), "+a"(acc[5]), "+a"(acc[6]), "+a"(acc[7])
#define KWM_WITH_ACC(STR)                                                                                      \
  do {                                                                                                         \
    static_assert(TM * TN == 8 || TM * TN == 9 || TM * TN == 12, "the operand lists are written out");        \
    if constexpr (TM * TN == 8) asm volatile(STR : KWM_ACC8::"memory");                                       \
    else if constexpr (TM * TN == 9) asm volatile(STR : KWM_ACC8, "+a"(acc[8])::"memory");                    \
    else asm volatile(STR : KWM_ACC8, "+a"(acc[8]), "+a"(acc[9]), "+a"(acc[10]), "+a"(acc[11])::"memory");    \
  } while (0)
  int ahead = 0;   // the tile `sa` / `sb` point at, relative to t_begin
  auto tile = [&](auto curc, int buf, int bnext) {
    constexpr int cur = decltype(curc)::value, nxt = cur ^ 1;
    const unsigned aimg = bnext * IMG_A * 8, bimg = bnext * IMG_B * 8;
    kw64_static_for<0, 4 * TM * TN>([&](auto ni) {
      constexpr int n = decltype(ni)::value;
      constexpr int s = n / (TM * TN), h = s / 2, e = s % 2, i = (n % (TM * TN)) / TN, jn = n % TN;
      double av, bv;
      if constexpr (!PA) av = ta2[cur][2 * i + h][e];
      else if constexpr (i < 2 * PAIRS_A) av = ta2[cur][s * PAIRS_A + i / 2][i % 2];
      else av = ta1[cur][s];
      if constexpr (!PB) bv = tb2[cur][2 * jn + h][e];
      else if constexpr (jn < 2 * PAIRS_B) bv = tb2[cur][s * PAIRS_B + jn / 2][jn % 2];
      else bv = tb1[cur][s];
      asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+a"(acc[i * TN + jn]) : "v"(av), "v"(bv));
      if constexpr (n < GA + GB) {
        dma(n, buf, std::integral_constant<int, NI>{});
        if constexpr (n == GA + GB - 1) {
          const bool more = ahead + 1 < nT;   // (scalar selects: the pointers stop at the wave's last tile)
          sa += more ? step_a : 0;
          sb += more ? step_b : 0;
          ahead += more ? 1 : 0;
          // the next tile's image has landed (the wave's own DMA: its vmcnt is all the ordering needed)
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GA + GB) : "memory");
        }
      } else if constexpr (n < GA + GB + RA + RB) {
        frag(nxt, aimg, bimg, std::integral_constant<int, n - (GA + GB)>{}, std::integral_constant<int, 1>{});
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    land(nxt);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("; @advance");   // (for the checker: the loop's t becomes t + 1)
    KWM_WITH_ACC("");
  };

  KWM_WITH_ACC("");
  if (nT > 0) {
    asm volatile("; @images %0 private" ::"n"(NI));
    // prologue: NI tiles in flight (a wave with fewer fetches its last tile again: the waits count instructions)
    kw64_static_for<0, NI>([&](auto ic) {
#pragma unroll
      for (int u = 0; u < GA + GB; ++u) dma(u, decltype(ic)::value, ic);
      const bool more = ahead + 1 < nT;
      sa += more ? step_a : 0;
      sb += more ? step_b : 0;
      ahead += more ? 1 : 0;
    });
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NI - 1) * (GA + GB)) : "memory");
    kw64_static_for<0, RA + RB>([&](auto ri) { frag(0, 0u, 0u, ri, std::integral_constant<int, 0>{}); });
    land(0);
    __builtin_amdgcn_sched_barrier(0);
    // (the fragment sets alternate by tile parity: two tiles a trip; an odd run -- only the wave that holds the end of K has
    //  one -- ends with a GHOST tile whose fragments are zero: a second instance of the body outside the loop makes the compiler
    //  shuttle the accumulators through VGPRs, tools/asm_acc_lint.py)
    static_assert(NI == 2, "two tiles a trip: an even tile's image is image 0");
    for (int t = 0; t < nT; t += 2) {
      tile(std::integral_constant<int, 0>{}, 0, 1);
      if (t + 1 >= nT) zero(1);
      tile(std::integral_constant<int, 1>{}, 1, 0);
    }
  }
  // The last MFMAs retire before anything but another MFMA touches the AccVGPRs (tools/asm_inflight_check.py rule 6)
  KWM_WITH_ACC("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15");
#undef KWM_WITH_ACC
#undef KWM_ACC8

  // the ragged end of K (fewer than 16): the last wave, operands straight from global memory, four k per MFMA
  if (g.K % BK != 0 && wave == NW - 1) {
    long ra[TM], cb[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const long m = m0 + kw64m_row_of<PA, TM>(i, l15);
      ra[i] = (m < g.M ? m : g.M - 1) * g.a_sm;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const long n = n0 + kw64m_row_of<PB, TN>(j, l15);
      cb[j] = (n < g.N ? n : g.N - 1) * g.b_sn;
    }
    for (int kk = KT * BK; kk < g.K; kk += 4) {
      const int k = kk + kg;
      const bool ok = k < g.K;
      const long kc = ok ? k : g.K - 1;
      double av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const double v = g.A[ra[i] + kc * g.a_sk];
        av[i] = ok ? v : 0.0;
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const double v = g.B[kc * g.b_sk + cb[j]];
        bv[j] = ok ? v : 0.0;
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i * TN + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i * TN + j], 0, 0, 0);
    }
  }

  // partial tiles -> LDS (each wave into its own, now dead, images), summed in wave order
  // D register r of lane (l15, kg): row kg + 4 r, column l15 of its block; block rows / columns back to the tile's by row_of
  {
    double* P = smem + wave * WAVE_DOUBLES;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = kw64m_row_of<PB, TN>(j, l15);
#pragma unroll
        for (int r = 0; r < 4; ++r) P[kw64m_row_of<PA, TM>(i, kg + 4 * r) * BN + col] = acc[i * TN + j][r];
      }
  }
  __syncthreads();
  auto finish = [&](auto plainc) {
    constexpr bool PLAIN = decltype(plainc)::value;
    for (int q = tid; q < BM * BN / 2; q += NW * 64) {
      const int row = q / (BN / 2), c2 = (q % (BN / 2)) * 2;
      f64x2 s = *reinterpret_cast<const f64x2*>(smem + row * BN + c2);
#pragma unroll
      for (int w = 1; w < NW; ++w) s += *reinterpret_cast<const f64x2*>(smem + w * WAVE_DOUBLES + row * BN + c2);
      const long gr = m0 + row, gc = n0 + c2;
      if (gr >= g.M || gc >= g.N) continue;
      double* dst = g.C + gr * g.c_sm + gc;
      if constexpr (PLAIN) {  // (wide: N % 2 == 0, a pair is in or out)
        *reinterpret_cast<f64x2*>(dst) = g.alpha * s;
      } else {
        double v[2] = {s.x, s.y};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          if (gc + e >= g.N) break;
          double x = g.alpha * v[e];
          if (g.cin) x += g.beta * g.cin[gr * g.c_sm + gc + e];
          if (g.bias) x += g.bias[gc + e];
          if (g.act == 1) x = dm::logistic(x);
          else if (g.act == 2) x = tanh(x);
          if (g.dact) {
            const double hh = g.dact[gr * g.c_sm + gc + e];
            x *= g.dact_kind ? 1.0 - hh * hh : hh * (1.0 - hh);
          }
          v[e] = x;
        }
        if (g.wide) {
          f64x2 o = {v[0], v[1]};
          *reinterpret_cast<f64x2*>(dst) = o;
        } else {
#pragma unroll
          for (int e = 0; e < 2; ++e)
            if (gc + e < g.N) dst[e] = v[e];
        }
      }
    }
  };
  if (g.wide && !g.bias && g.act == 0 && !g.dact && !g.cin) finish(std::true_type{});
  else finish(std::false_type{});
}

// to_set_gemm_f64_menu: 0 off (default), 1 where the scan found it ahead, 2 wherever kw64_menu_can holds; tile -1 / a menu index
static int g_kw64m_mode = 0, g_kw64m_tile = -1;

bool gemm_kw64_menu_set(int mode, int tile, int* previous_mode) {
  if (mode < 0 || mode > 2 || tile < -1 || tile >= KW64M_TILES) return false;
  if (previous_mode) *previous_mode = g_kw64m_mode;
  g_kw64m_mode = mode;
  g_kw64m_tile = tile;
  return true;
}

// gemm_kw64_kernel's problem class (kw64_can: same operand rules, the same 32-bit DMA offsets); a K tail rides in the kernel
// -- from one block of rows and columns on: a single (padded) tile is a legal launch; loads clamp, stores are guarded
static bool kw64_menu_can(const GemmProblem& p) {
  if (p.dtype != TO_F64 || p.batch != 1 || p.reduce_batch || p.rowsum || p.loss_rows || p.tail_out || p.a_table || (p.beta != 0.0 && !p.Cin)) return false;
  if (p.M < 16 || p.N < 16 || p.K < 16) return false;
  if (p.M > 2147483647LL || p.N > 2147483647LL || p.K > 2147483647LL) return false;
  const bool a_k = p.a_sk == 1, a_m = !a_k && p.a_sm == 1;
  const bool b_n = p.b_sn == 1, b_k = !b_n && p.b_sk == 1;
  if (!(a_k || a_m) || !(b_n || b_k)) return false;
  auto al8 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7u) == 0; };
  if (!al8(p.A) || !al8(p.B)) return false;
  const int64_t ext_a = a_k ? p.M * p.a_sm : 16 * p.a_sk + p.M, ext_b = b_k ? p.N * p.b_sn : 16 * p.b_sk + p.N;
  if (ext_a * 8 + 8192 >= (1LL << 32) || ext_b * 8 + 8192 >= (1LL << 32) || p.a_sm < 0 || p.a_sk < 0 || p.b_sk < 0 || p.b_sn < 0) return false;
  if (a_m && p.M % 2 != 0) return false;  // an m-contiguous pair must be in or out of the matrix as a whole
  if (b_n && p.N % 2 != 0) return false;
  return true;
}

// The cost rule, fitted to profiles/gemm_f64_menu_scan.txt (tools/gemm_f64_menu_scan.py): a launch costs 3.2 us + (rounds of the
// 256 CUs: one workgroup a CU, 96 .. 112 KiB of LDS) x (k-tiles) x (a k-tile's MFMA time on the tile: 4 TM TN MFMAs of 64 cycles
// over four SIMDs at 2.4 GHz) / 0.824.  Model / measured us: 768^3 on 48x48 17.2 / 17.2, 1536^3 115.1 / 115.1 (the two it was
// fitted on), 1280^3 73.1 / 72.6, 640^3 on 64x32 13.6 / 13.3, 1024 x 1024 x 512 19.8 / 19.0, 1088^3 on 48x64 56.0 / 56.5,
// 768 x 1024 x 1024 28.1 / 27.2, 1152 x 2048 x 1152 102.6 / 93.7.  It is optimistic past four rounds and under short K (60000 x
// 300 x 100 on 48x64: 77 / 117; 8192 x 300 x 100 on 32x64: 13.0 / 17.8 -- five k-tiles a wave do not pay for prologue and
// reduction): more than 1,024 tiles cost infinity here, and mode 1 asks for K >= 512.
static const double KW64M_LAUNCH_US = 3.2, KW64M_EFF = 0.824;
static double kw64m_cost(const GemmProblem& p, const Kw64mShape& s) {
  const long T = ((p.M + 16 * s.tm - 1) / (16 * s.tm)) * ((p.N + 16 * s.tn - 1) / (16 * s.tn)), KT = (p.K + 15) / 16;
  if (T > 4 * 256) return 1e30;
  const long rounds = (T + 255) / 256;
  return KW64M_LAUNCH_US + (double)rounds * KT * (s.tm * s.tn * 64.0 / 2400.0) / KW64M_EFF;
}
// Mode 1: a SCANNED shape (M, K, N of profiles/gemm_f64_menu_scan.txt, with the us of the route it takes today -- the scan's
// mode0 column, equal to the parent's within 0.3 % -- and the menu tile the scan measured fastest, its `best` column) whose
// modelled time on that tile is below today's measured time by the MARGIN.  The largest run-to-run spread the scan saw on either
// side was 0.033 (1536^3); the margin is 0.07, twice that.  (The scan is the house protocol of tools/gemm_scan.py: three passes of
// 20 ms windows, the parent in a child process ahead of each pass, not alternated shape by shape -- short windows also measure
// the clock and the scheduler, which is one more reason for a margin of twice the spread and for a switch that is off by default.)
// That takes 640^3 (23.1 -> 13.3 us measured), 768^3 (26.9 -> 17.2), 1088^3 (69.0 -> 56.5), 1152^3 (72.3 -> 56.5), 1280^3 (80.1
// -> 72.6), 1536^3 (178.2 -> 109.8), 768 x 1024 x 1024 (34.1 -> 27.2), 1024 x 1024 x 512 (33.7 -> 19.0), 1152 x 2048 x 1152
// (121.2 -> 93.7) and nothing else: 896^3, 1000^3, 1024^3, 2048^3, 3072^3, 4096 x 784 x 256, the long-K few-tile shapes and the
// Learn shapes measured behind or level.  Every shape the scan did not time keeps today's route.
struct Kw64mScanned { int m, k, n; double today_us; int tile; };
static const Kw64mScanned kw64m_scanned[] = {
    {640, 640, 640, 23.1, 4}, {768, 768, 768, 26.9, 0}, {896, 896, 896, 30.7, 4}, {1000, 1000, 1000, 34.8, 4},
    {1024, 1024, 1024, 34.4, 4}, {1088, 1088, 1088, 69.0, 1}, {1152, 1152, 1152, 72.3, 1}, {1280, 1280, 1280, 80.1, 0},
    {1536, 1536, 1536, 178.2, 1}, {2048, 2048, 2048, 237.9, 4}, {3072, 3072, 3072, 813.6, 1}, {768, 1024, 1024, 34.1, 1},
    {4096, 784, 256, 29.1, 4}, {1024, 1024, 512, 33.8, 4}, {512, 2048, 512, 27.5, 3}, {384, 4096, 384, 50.1, 3},
    {1152, 2048, 1152, 121.3, 1}, {60000, 784, 300, 490.5, 1}, {60000, 300, 100, 97.4, 1}, {8192, 300, 100, 15.1, 3},
    {8192, 100, 300, 23.8, 3}, {100, 8192, 300, 95.4, 3}, {100, 60000, 300, 673.6, 3}};
static const double KW64M_MARGIN = 0.07;
static const Kw64mScanned* kw64m_scanned_row(const GemmProblem& p) {
  for (const Kw64mScanned& r : kw64m_scanned)
    if (r.m == p.M && r.k == p.K && r.n == p.N) return &r;
  return nullptr;
}
// The tile: the forced one; on a scanned shape the one the scan measured fastest (the model ties where two tiles come to the
// same rounds x MFMAs -- 1536^3: 4 rounds of 48x48 and 3 of 48x64 are both 92.16 us of MFMA time, measured 115.1 and 109.8);
// elsewhere (mode 2 only) the model's cheapest, the first of equals.
static int kw64m_pick(const GemmProblem& p) {
  if (g_kw64m_tile >= 0) return g_kw64m_tile;
  if (const Kw64mScanned* r = kw64m_scanned_row(p)) return r->tile;
  int best = 0;
  for (int i = 1; i < KW64M_TILES; ++i)
    if (kw64m_cost(p, kw64m_menu[i]) < kw64m_cost(p, kw64m_menu[best])) best = i;
  return best;
}
static bool kw64m_auto(const GemmProblem& p) {
  if (p.K < 512) return false;
  const Kw64mScanned* r = kw64m_scanned_row(p);
  return r && kw64m_cost(p, kw64m_menu[kw64m_pick(p)]) < (1.0 - KW64M_MARGIN) * r->today_us;
}

bool gemm_kw64_menu_applicable(const GemmProblem& p) {
  if (g_kw64m_mode == 0 || !kw64_menu_can(p)) return false;
  return g_kw64m_mode == 2 || kw64m_auto(p);
}

bool gemm_kw64_menu_everywhere(const GemmProblem& p) { return g_kw64m_mode == 2 && kw64_menu_can(p); }

template <int TM, int TN>
static void kw64m_launch_modes(int mode, dim3 grid, hipStream_t s, const Kw64Args& g) {
  switch (mode) {
    case 0: launch_k((gemm_kw64_menu_kernel<0, 0, TM, TN>), grid, dim3(256), 0, s, g); break;
    case 1: launch_k((gemm_kw64_menu_kernel<0, 1, TM, TN>), grid, dim3(256), 0, s, g); break;
    case 2: launch_k((gemm_kw64_menu_kernel<1, 0, TM, TN>), grid, dim3(256), 0, s, g); break;
    default: launch_k((gemm_kw64_menu_kernel<1, 1, TM, TN>), grid, dim3(256), 0, s, g); break;
  }
}

void launch_gemm_kw64_menu(const GemmProblem& p, hipStream_t s) {
  const Kw64mShape sh = kw64m_menu[kw64m_pick(p)];
  Kw64Args g{};
  g.A = (const double*)p.A; g.B = (const double*)p.B; g.C = (double*)p.C;
  g.M = (int)p.M; g.N = (int)p.N; g.K = (int)p.K;
  g.a_sm = p.a_sm; g.a_sk = p.a_sk; g.b_sk = p.b_sk; g.b_sn = p.b_sn; g.c_sm = p.c_sm;
  g.tiles_m = (int)((p.M + 16 * sh.tm - 1) / (16 * sh.tm));
  g.tiles_n = (int)((p.N + 16 * sh.tn - 1) / (16 * sh.tn));
  g.alpha = p.alpha;
  g.bias = (const double*)p.bias; g.dact = (const double*)p.dact; g.act = p.act; g.dact_kind = p.dact_kind;
  g.cin = p.beta != 0.0 ? (const double*)p.Cin : nullptr; g.beta = (double)p.beta;
  g.wide = (reinterpret_cast<uintptr_t>(p.C) & 15u) == 0 && p.c_sm % 2 == 0 && p.N % 2 == 0;
  const int mode = (p.a_sk == 1 ? 0 : 2) + (p.b_sn == 1 ? 0 : 1);
  const dim3 grid(g.tiles_m * g.tiles_n);
  if (sh.tm == 3 && sh.tn == 3) kw64m_launch_modes<3, 3>(mode, grid, s, g);
  else if (sh.tm == 3 && sh.tn == 4) kw64m_launch_modes<3, 4>(mode, grid, s, g);
  else if (sh.tm == 4 && sh.tn == 3) kw64m_launch_modes<4, 3>(mode, grid, s, g);
  else if (sh.tm == 2 && sh.tn == 4) kw64m_launch_modes<2, 4>(mode, grid, s, g);
  else kw64m_launch_modes<4, 2>(mode, grid, s, g);
  TO_HIP(hipGetLastError());
  count_launch();
}

}  // namespace to
