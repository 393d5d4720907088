// Tool kit of the two KAN kernel sets (kan.hip: grid_size 5 at compile-time sizes; kan_general.hip: any
// grid size as a launch argument, and the refit): the basis recursion, the chunk and tile helpers, the
// MFMA loop, the slab reduction, and the host-side partitions that both sets launch by.
#pragma once
#include "siren_common.h"
#include "siren_kernels.h"

// KAN_ABL (measurement-only builds via tools/kan_ablate.py, never the product): bit 1 replaces
// the basis recursion by a trivial stand-in, bit 2 skips the chunk products.
#ifndef KAN_ABL
#define KAN_ABL 0
#endif
// knot window of the basis recursion (kan_bases_window): 1 = span by counting + an 8-knot gather
// from the LDS knot row (cfg5 2.249 -> 2.202 ms per step), 0 = per-span predicate with the window
// captured by selects (kept for the head kernels, whose lanes hold one input's knots throughout)
#ifndef KAN_WINDOW_GATHER
#define KAN_WINDOW_GATHER 1
#endif

namespace siren {

constexpr int KAN_NG = 12;  // grid knots per input: grid_size + 2 * spline_order + 1 (KAN_NB, KAN_K1: siren_kernels.h)

// Cox-de Boor recursion of kan.py:94-104 for one x on one input's knots g[0..11]: order-0
// bases B[j] = (g[j] <= x < g[j+1]), then for k = 1..3
//   B[j] = ((x - g[j]) / (g[j+k] - g[j])) * B[j] + ((g[j+k+1] - x) / (g[j+k+1] - g[j+1])) * B[j+1]
// (each product rounded, then the sum: fp-contract off), and with DERIV the recursion
// differentiated in x.
// Evaluated on its support only.  An order-0 basis is 1 on at most one
// knot span s (g[s] <= x < g[s+1], the same predicate), so after step k only B[s-k .. s] can be
// non-zero; every other term of the full recursion is l*0 + r*0 = +-0 and, where it meets a
// non-zero term, x + (+-0) = x.  Computing the window terms with the same operations in the
// same order therefore gives the full recursion's values bit for bit (zeros up to sign), at 18
// instead of 54 divisions (36 instead of 108 with the derivative).
// The span search also captures the lane's knot window kw[d] = g[s-3+d] (d = 0..7) with selects,
// so the recursion indexes registers statically: no per-lane knot gathers.  Terms whose knot
// index falls outside the array are computed on stale window entries and discarded by a select
// (the full recursion has no such term).
// Forward (RCP false): every quotient a / D is the correctly rounded one, without a division:
// with y = RN(1/D) from the per-input table inv[(k-1)*11 + j] = 1 / (g[j+k] - g[j]) (IEEE
// divisions, once per input: kf_fill_inv), q = RN(a y), r = a - D q (exact by fma) and
// q' = RN(q + r y) equals RN(a / D) (Markstein's theorem: y within half an ulp of 1/D, q within
// one ulp of a/D; no underflow or overflow on these knot grids), so the bases stay bit-identical
// to torch's (tests/test_gpu_kan.py::test_kan_forward_bases_bit_exact).
// RCP (backward kernels): the knot-difference divisions become products with v_rcp_f32
// reciprocals (within an ulp of the divisions; only the weight / input gradients see them).
__device__ __forceinline__ float kan_div(float a, float d, float y) {
  const float q = a * y;
  const float r = fmaf(-q, d, a);
  return fmaf(r, y, q);
}

// How kan_bases_window finds the span: by a count over the 12 knots of grid 5 (KAN_WINDOW_GATHER),
// by grid 5's per-span predicate with the window captured by selects, or by bisection on a
// run-time number of knots (kan_general.hip)
enum { KAN_SPAN_COUNT = 0, KAN_SPAN_SELECT = 1, KAN_SPAN_BISECT = 2 };
constexpr int KAN_SPAN_5 = KAN_WINDOW_GATHER != 0 ? KAN_SPAN_COUNT : KAN_SPAN_SELECT;

// The span s of x on an input's ng knots g (-1 outside the grid), its knot window
// kw[e] = g[s-3+e], and the recursion on the window: w[q] = B[s-3+q] and, with DERIV,
// d[q] = B'[s-3+q] (q = 0..3).  One recursion for both kernel sets: the same operations in the same
// order, so the same bits.  ng is KAN_NG at compile time unless SPAN is KAN_SPAN_BISECT; inv is the
// input's table inv[(k-1)(ng-1) + j] = RN(1 / (g[j+k] - g[j])).  Slots whose basis index s-3+q
// falls outside 0 .. ng-5 hold values of discarded terms: the callers skip them.
// (The span search and the recursion stay one function: as a callee of its own the recursion is
// simplified before it meets the span's range, and every grid-5 kernel compiled differently.)
template <bool DERIV, bool RCP, int SPAN>
__device__ __forceinline__ int kan_bases_window(float x, const float* __restrict__ g, int ng_rt, float* w, float* d,
                                                const float* __restrict__ inv) {
  const int ng = SPAN == KAN_SPAN_BISECT ? ng_rt : KAN_NG;
  int s = -1;
  float kw[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if constexpr (SPAN != KAN_SPAN_SELECT) {
    // for non-decreasing knots, g[s] <= x < g[s+1] holds exactly for s = #{j : g[j] <= x} - 1 when
    // that count is 1 .. ng-1 (x below the first knot, at or past the last one, or NaN: no span),
    // the same s as the per-span predicate below.  The count: over all knots, or the place where
    // x >= g[j] turns false, found by bisection (a NaN fails every comparison: count 0).  The
    // window is then one gather of 8 knots from the LDS row g (indices clamped into the array; the
    // entries a clamp touches belong to terms the recursion discards)
    int cnt = 0;
    if constexpr (SPAN == KAN_SPAN_COUNT) {
#pragma unroll
      for (int j = 0; j < KAN_NG; ++j) cnt += (x >= g[j]) ? 1 : 0;
    } else {
      int hi = ng;
      while (cnt < hi) {
        const int mid = (cnt + hi) >> 1;
        if (x >= g[mid]) cnt = mid + 1;
        else hi = mid;
      }
    }
    s = (cnt >= 1 && cnt <= ng - 1) ? cnt - 1 : -1;
    const int s0 = s < 0 ? 0 : s;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int t = s0 - 3 + e;
      t = t < 0 ? 0 : (t > ng - 1 ? ng - 1 : t);
      kw[e] = g[t];
    }
  } else {
    float kn[KAN_NG];
#pragma unroll
    for (int j = 0; j < KAN_NG; ++j) kn[j] = g[j];
#pragma unroll
    for (int j = 0; j < KAN_NG - 1; ++j) {
      const bool hit = x >= kn[j] && x < kn[j + 1];
      s = hit ? j : s;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int t = j - 3 + e;
        if (t >= 0 && t < KAN_NG) kw[e] = hit ? kn[t] : kw[e];
      }
    }
  }
  // window w[q] = B[s - 3 + q], q = 0..3, plus w[4] = B[s + 1] = 0
  float ww[5] = {0.0f, 0.0f, 0.0f, 1.0f, 0.0f}, dd[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 1; k <= 3; ++k) {
#pragma unroll
    for (int q = 3 - k; q < 4; ++q) {
      const int j = s - 3 + q;
      const bool ok = j >= 0 && j <= ng - 2 - k;  // inside the support and the array
      const float gj = kw[q], gjk = kw[q + k], gj1 = kw[q + 1], gjk1 = kw[q + k + 1];
      float il, ir, l, r;
      if constexpr (RCP) {
        il = __builtin_amdgcn_rcpf(gjk - gj);
        ir = __builtin_amdgcn_rcpf(gjk1 - gj1);
        l = (x - gj) * il;
        r = (gjk1 - x) * ir;
      } else {
        const int jt = j < 0 ? 0 : (j > ng - 2 - k ? ng - 2 - k : j);  // in-table for discarded terms
        il = inv[(k - 1) * (ng - 1) + jt];
        ir = inv[(k - 1) * (ng - 1) + jt + 1];
        l = kan_div(x - gj, gjk - gj, il);
        r = kan_div(gjk1 - x, gjk1 - gj1, ir);
      }
      if constexpr (DERIV) {
        const float nd = il * ww[q] + l * dd[q] - ir * ww[q + 1] + r * dd[q + 1];
        dd[q] = ok ? nd : dd[q];
      }
      const float nw = l * ww[q] + r * ww[q + 1];
      ww[q] = ok ? nw : ww[q];
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    w[q] = ww[q];
    if constexpr (DERIV) d[q] = dd[q];
  }
  return s;
}

template <bool DERIV, bool RCP = false, int SPAN = KAN_SPAN_5>
__device__ __forceinline__ void kan_bases_local(float x, const float* __restrict__ g, float* b, float* db,
                                                const float* __restrict__ inv = nullptr) {
#pragma unroll
  for (int j = 0; j < KAN_NB; ++j) b[j] = db[j] = 0.0f;
  if constexpr ((KAN_ABL & 1) != 0) {
#pragma unroll
    for (int j = 0; j < KAN_NB; ++j) b[j] = db[j] = x * g[j];
    return;
  }
  float w[4], d[4];
  const int s = kan_bases_window<DERIV, RCP, SPAN>(x, g, KAN_NG, w, d, inv);
  if (s < 0) return;
#pragma unroll
  for (int c = 0; c < KAN_NB; ++c) {
    // B[c] = w[c - s + 3] when that is a window slot
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool at = (c == s - 3 + q);
      b[c] = at ? w[q] : b[c];
      if constexpr (DERIV) db[c] = at ? d[q] : db[c];
    }
  }
}

__device__ __forceinline__ float silu(float x) { return x / (1.0f + expf(-x)); }
// silu(x) and its derivative on one exp (a caller that needs the derivative alone drops sl)
__device__ __forceinline__ void silu_and_grad(float x, float& sl, float& dsl) {
  const float d = 1.0f + expf(-x);
  sl = x / d;
  const float s = 1.0f / d;
  dsl = s * (1.0f + x * (1.0f - s));
}

// ---- fused layer kernels --------------------------------------------------------------------
// Chunk of IC inputs i0 .. i0+ic-1 (ic <= IC): local column kk < ic is the SiLU column of input
// i0+kk (combined-weight column k = i0+kk), kk = ic + 8 ii + c the spline basis c of input i0+ii
// (k = in + 8 (i0+ii) + c).  kc = 9 ic columns, padded to kpad (a multiple of 16) with zeros.
// The products run on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fmaf chain; the same rate
// as the f32 VALU but one LDS operand per 2048 flops instead of per 2): lane l supplies
// A[l&15][k=l>>4] and B[k=l>>4][l&15]; D[row=(l>>4)*4+reg][col=l&15].
constexpr int KF_IC = 16, KF_KC = 9 * KF_IC, KF_R = 64, KF_O = 64;
constexpr int64_t kKanResidentBlocks = 512;     // 256 CUs x 2 (LDS-limited) for the fused kernels
constexpr int64_t kKanBwdResidentBlocks = 256;  // kan_bwd_fused: one 512-thread block per CU

struct KfChunk {
  int i0, ic, kc, kpad, nkt;  // first input, inputs, columns, columns padded to 16, 16-column tiles
  // combined-weight column of local column kk < kc
  __device__ __forceinline__ int col(int kk, int in) const { return kk < ic ? i0 + kk : in + 8 * i0 + (kk - ic); }
};
__device__ __forceinline__ KfChunk kf_chunk(int i0, int in) {
  const int ic = in - i0 < KF_IC ? in - i0 : KF_IC, kc = KAN_K1 * ic, kpad = (kc + 15) & ~15;
  return KfChunk{i0, ic, kc, kpad, kpad >> 4};
}

__device__ __forceinline__ f32x4 kf_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Xs[r][ii] = X[r0 + r][i0 + ii] for rows < re (else 0): the chunk's inputs, read along the row
// (a full chunk with in % 4 == 0: one 16-byte load per thread).  All tile loaders below issue
// every load of the tile before the first LDS store, so a tile costs one memory latency.
__device__ __forceinline__ float4 ldg4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ void kf_stage_x(float (*Xs)[KF_IC + 1], const float* __restrict__ X, int64_t re, int in,
                                           int64_t r0, int i0, int ic) {
  if (ic == KF_IC && (in & 3) == 0) {
    if (threadIdx.x < KF_R * KF_IC / 4) {
      const int r = threadIdx.x >> 2, i4 = (threadIdx.x & 3) * 4;
      float4 v = float4{0.f, 0.f, 0.f, 0.f};
      if (r0 + r < re) v = ldg4(X + (r0 + r) * in + i0 + i4);
      Xs[r][i4] = v.x;
      Xs[r][i4 + 1] = v.y;
      Xs[r][i4 + 2] = v.z;
      Xs[r][i4 + 3] = v.w;
    }
    return;
  }
  for (int e = threadIdx.x; e < KF_R * KF_IC; e += blockDim.x) {
    const int r = e / KF_IC, ii = e % KF_IC;
    const int64_t n = r0 + r;
    Xs[r][ii] = (n < re && ii < ic) ? X[n * in + i0 + ii] : 0.f;
  }
}

// gk[ii][j] = knot j of input i0 + ii.  The recursion reads knots at a per-row span index; from
// LDS those reads cost an LDS round trip, from global memory an L1/L2 one on every step.
constexpr int KF_GST = KAN_NG + 1;
__device__ __forceinline__ void kf_fill_knots(float (*gk)[KF_GST], const float* __restrict__ grid, int i0, int ic) {
  for (int e = threadIdx.x; e < ic * KAN_NG; e += blockDim.x) gk[e / KAN_NG][e % KAN_NG] = grid[i0 * KAN_NG + e];
}

// inv[ii][(k-1)*11 + j] = RN(1 / (g[j+k] - g[j])) for the knots of inputs i0 .. i0+ic-1 (IEEE
// divisions; the forward's exact quotients, kan_div)
constexpr int KF_VST = 33;
__device__ __forceinline__ void kf_fill_inv(float (*inv)[KF_VST], const float* __restrict__ grid, int i0, int ic) {
  for (int e = threadIdx.x; e < ic * 33; e += blockDim.x) {
    const int ii = e / 33, q = e - ii * 33, k = q / 11 + 1, j = q - (k - 1) * 11;
    const float* g = grid + (i0 + ii) * KAN_NG;
    inv[ii][q] = (j + k < KAN_NG) ? 1.0f / (g[j + k] - g[j]) : 0.0f;
  }
}

// Operand tiles are read with one ds_read_b128 per lane per 16-k group: lane group lk = l>>4
// supplies k = 16 g + 4 lk + t to the t-th MFMA of group g (a permutation of the summation index
// applied to both operands alike).  Row strides are 4 mod 32 floats, so each 8-lane phase of a
// b128 read covers the 32 banks once.  The next group's fragments are loaded while the current
// group's MFMAs issue.
constexpr int KF_AST = KF_KC + 4;  // [row][kk] tiles of the forward
constexpr int KF_CST = KF_R + 4;   // [*][row] / [*][o] tiles of the backward
constexpr int KF_DST = KF_KC + 1;  // dA rows [r][kk] of the backward

// ---- tile helpers of the backward kernels (blocks of T = 256 or 512 threads) ------------------
// As[kk][r] (stride KF_CST) = A columns of the chunk for rows r0 + r (zero past re, and rows
// kc .. kpad-1 zero), v_rcp_f32 quotients.  A wave takes one input ii and 64 consecutive rows: its
// knots are uniform and the LDS writes are conflict-free.  The pair p of a block is (r, ii) =
// (p & 63, p >> 6): kf_da_to_gin numbers them alike.  (kan_bwd_fused fills its A tile itself, with
// the derivatives kept in registers: through this helper its products measured 0.9 % slower.)
__device__ __forceinline__ void kf_fill_a(float (*As)[KF_CST], const float (*Xs)[KF_IC + 1], const float (*gk)[KF_GST],
                                          int64_t re, int64_t r0, const KfChunk& ch) {
  for (int p = threadIdx.x; p < KF_R * ch.ic; p += blockDim.x) {
    const int r = p & (KF_R - 1), ii = p >> 6;
    float b[KAN_NB], unused[KAN_NB], sl = 0.f;
    if (r0 + r < re) {
      const float x = Xs[r][ii];
      kan_bases_local<false, true>(x, gk[ii], b, unused);
      sl = silu(x);
    } else {
#pragma unroll
      for (int c = 0; c < KAN_NB; ++c) b[c] = 0.f;
    }
    As[ii][r] = sl;
#pragma unroll
    for (int c = 0; c < KAN_NB; ++c) As[ch.ic + 8 * ii + c][r] = b[c];
  }
  for (int e = threadIdx.x; e < (ch.kpad - ch.kc) * KF_R; e += blockDim.x) As[ch.kc + e / KF_R][e % KF_R] = 0.f;
}

// G tile: 64 rows from r0 (zero past re) x 64 outs from oc of G[N][out], as Gl[r][o] or, TRANSPOSED,
// Gl[o][r] (stride KF_CST).  In float4 pieces when out % 4 == 0 and the 64 outs exist: the thread's
// piece q is idx = tid + T q; BY_ROW: lanes take consecutive rows (r = idx & 63, outs 4 (idx >> 6):
// conflict-free transposed stores), else consecutive pieces of a row (r = idx >> 4, outs 4 (idx & 15)).
// Loading to registers and storing to LDS are separate calls, so a tile costs one memory latency
// and the next tile's loads can go out under the current tile's products.
template <int T>
using KfGRegs = float4[KF_R * KF_O / 4 / T];

template <int T, bool BY_ROW>
__device__ __forceinline__ void kf_g_piece(int q, int& r, int& o4) {
  const int idx = threadIdx.x + T * q;
  r = BY_ROW ? idx & 63 : idx >> 4;
  o4 = BY_ROW ? idx >> 6 : idx & 15;
}

template <int T, bool BY_ROW>
__device__ __forceinline__ void kf_g_load(KfGRegs<T>& v, const float* __restrict__ G, int64_t re, int out, int64_t r0,
                                          int oc) {
#pragma unroll
  for (int q = 0; q < KF_R * KF_O / 4 / T; ++q) {
    int r, o4;
    kf_g_piece<T, BY_ROW>(q, r, o4);
    v[q] = r0 + r < re ? ldg4(G + (r0 + r) * out + oc + 4 * o4) : float4{0.f, 0.f, 0.f, 0.f};
  }
}

template <int T, bool BY_ROW, bool TRANSPOSED>
__device__ __forceinline__ void kf_g_store(float* Gl, const KfGRegs<T>& v) {
#pragma unroll
  for (int q = 0; q < KF_R * KF_O / 4 / T; ++q) {
    int r, o4;
    kf_g_piece<T, BY_ROW>(q, r, o4);
    if constexpr (TRANSPOSED) {
      Gl[(4 * o4) * KF_CST + r] = v[q].x;
      Gl[(4 * o4 + 1) * KF_CST + r] = v[q].y;
      Gl[(4 * o4 + 2) * KF_CST + r] = v[q].z;
      Gl[(4 * o4 + 3) * KF_CST + r] = v[q].w;
    } else {
      *reinterpret_cast<float4*>(Gl + r * KF_CST + 4 * o4) = v[q];
    }
  }
}

// any out and oc: element by element, bounds-checked (lanes along the rows or along the outs)
template <int T, bool BY_ROW, bool TRANSPOSED>
__device__ __forceinline__ void kf_g_scalar(float* Gl, const float* __restrict__ G, int64_t re, int out, int64_t r0,
                                            int oc) {
  for (int e = threadIdx.x; e < KF_R * KF_O; e += T) {
    const int r = BY_ROW ? e % KF_R : e / KF_O, o = BY_ROW ? e / KF_R : e % KF_O;
    Gl[TRANSPOSED ? o * KF_CST + r : r * KF_CST + o] = (r0 + r < re && oc + o < out) ? G[(r0 + r) * out + oc + o] : 0.f;
  }
}

// Wl[kk][o] (stride KF_CST) = W[oc + o][col(kk)] through the transposed copy WT[9 in][out] (rows
// along o: coalesced, no conflicts); rows kc .. kpad-1 and the outs past `out` are zero.  vec (256
// threads, a full chunk with in % 4 == 0, out % 4 == 0 and the 64 outs exist): 9 float4 pieces a thread.
template <int T>
__device__ __forceinline__ void kf_load_wt(float* Wl, const float* __restrict__ WT, const KfChunk& ch, int in, int out,
                                           int oc, bool vec) {
  if constexpr (T * 9 == KF_KC * KF_O / 4) {
    if (vec) {
      float4 v[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const int idx = threadIdx.x + T * q, kk = idx >> 4, o4 = idx & 15;
        v[q] = ldg4(WT + (int64_t)ch.col(kk, in) * out + oc + 4 * o4);
      }
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const int idx = threadIdx.x + T * q, kk = idx >> 4, o4 = idx & 15;
        *reinterpret_cast<float4*>(Wl + kk * KF_CST + 4 * o4) = v[q];
      }
      return;
    }
  }
  for (int e = threadIdx.x; e < ch.kpad * KF_O; e += T) {
    const int kk = e / KF_O, o = e % KF_O;
    Wl[kk * KF_CST + o] = (kk < ch.kc && oc + o < out) ? WT[(int64_t)ch.col(kk, in) * out + oc + o] : 0.f;
  }
}

// dA -> Gin.  The wave's dA accumulators (acc[j][q]: row `row` + q, column `col` + 16 j, j < nj) go
// to LDS as dAs[r][kk] (stride KF_DST) over the operand tile they came from, whose reads the
// caller's barrier has ended (columns past kc hold products of zero-padded W rows and are never
// read); the thread's pair h, p = tid + T h in kf_fill_a's numbering, contracts its row,
//   Gin[n][i] = SiLU'(x) dA[n][i] + sum_c B'_c(x) dA[n][in + 8 i + c],
// with the caller's dsl[h] = SiLU' and db[h][] = B' (REGS: kan_bwd_fused, the pair loop unrolled)
// or with the derivatives recomputed from Xs and gk, into Xs[r][ii] -- the element that thread
// alone reads -- and the X tile leaves as coalesced row segments.  The caller's next barrier frees
// Xs and dAs for refilling.
template <int T, bool REGS, int NA>
__device__ __forceinline__ void kf_da_to_gin(float* dAs, float (*Xs)[KF_IC + 1], const float (*gk)[KF_GST],
                                             const f32x4 (&acc)[NA], int nj, int row, int col, int64_t re, int64_t r0,
                                             int in, const KfChunk& ch, const float* dsl, const float (*db)[KAN_NB],
                                             float* __restrict__ Gin) {
#pragma unroll
  for (int j = 0; j < NA; ++j)
    if (j < nj)
#pragma unroll
      for (int q = 0; q < 4; ++q) dAs[(row + q) * KF_DST + col + 16 * j] = acc[j][q];
  __syncthreads();
  constexpr int NH = KF_R * KF_IC / T;
#pragma unroll REGS ? NH : 1
  for (int h = 0; h < NH; ++h) {
    const int p = threadIdx.x + T * h, r = p & (KF_R - 1), ii = p >> 6;
    if (ii >= ch.ic || r0 + r >= re) continue;
    float b[KAN_NB], dbl[KAN_NB], sl, ds;
    if constexpr (REGS) {
      ds = dsl[h];
    } else {
      const float x = Xs[r][ii];
      kan_bases_local<true, true>(x, gk[ii], b, dbl);
      silu_and_grad(x, sl, ds);
    }
    const float* dA = dAs + r * KF_DST;
    float v = ds * dA[ii];
#pragma unroll
    for (int c = 0; c < KAN_NB; ++c) v += (REGS ? db[h][c] : dbl[c]) * dA[ch.ic + 8 * ii + c];
    Xs[r][ii] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < KF_R * ch.ic; e += T) {
    const int r = e / ch.ic, ii = e - r * ch.ic;
    if (r0 + r < re) Gin[(r0 + r) * in + ch.i0 + ii] = Xs[r][ii];
  }
}

// The 1-D grids of the split-K kernels hold per * zpad blocks (per chunk tiles, zpad = splits
// rounded up to 8), numbered so that the blocks of one split (which read the same rows of G and X)
// share an XCD: block L runs on XCD L % 8.  -> the block's chunk tile cid and split z (>= splits
// for the padding blocks, which leave at once).
__device__ __forceinline__ void kf_split_block(int per, int& cid, int& z) {
  const int L = blockIdx.x, q8 = L >> 3;
  cid = q8 % per;
  z = (q8 / per) * 8 + (L & 7);
}

// slab[z][o + q][col(kk)] = acc[j][q] for the wave's dW accumulators: outs o .. o + 3, local
// columns kk = kk0 + 16 j (j < nj); ch: a KfChunk, or kan_general.hip's KgChunk with its k1
template <int NA, class Chunk>
__device__ __forceinline__ void kf_store_slab(float* __restrict__ slab, int z, const f32x4 (&acc)[NA], int nj, int kk0,
                                              int o, const Chunk& ch, int in, int out, int k1 = KAN_K1) {
  const int64_t K = (int64_t)k1 * in;
  float* out_slab = slab + (int64_t)z * out * K;
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int kk = kk0 + 16 * j;
    if (j >= nj || kk >= ch.kc) continue;
    const int64_t col = ch.col(kk, in);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (o + q < out) out_slab[(int64_t)(o + q) * K + col] = acc[j][q];
  }
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float f4(const float4& v, int t) { return t == 0 ? v.x : t == 1 ? v.y : t == 2 ? v.z : v.w; }

// acc[j] += sum over ng groups of 16 k: A(16 rows at ap) x B(16 cols at bp + j * bstride).
// Two accumulator sets (k-steps t = 0, 2 of a group into acc, t = 1, 3 into acc2, added at the
// end in that fixed order): 2 NJ independent MFMA chains per wave.  With NJ = 4 chains the f32
// MFMA's dependent-issue latency is exposed (tools/micro/mfma_f32_rate: 111 vs 146 TFLOP/s for 4
// vs 9 chains at two waves per SIMD).  SPLIT = false keeps one set (the forward: measured no gain,
// cfg5 kan_fwd 0.753 vs 0.778 ms per step; the backward products gain 4% of the step).
template <int NJ, int NA, bool SPLIT = true>
__device__ __forceinline__ void kf_mfma_groups(const float* ap, const float* bp, int bstride, int ng, f32x4 (&acc)[NA]) {
  static_assert(NJ <= NA, "more column tiles than accumulators");
  f32x4 acc2[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc2[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 a = ld4(ap), b[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) b[j] = ld4(bp + j * bstride);
  for (int g = 0; g < ng; ++g) {
    float4 an = a, bn[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bn[j] = b[j];
    if (g + 1 < ng) {
      an = ld4(ap + 16 * (g + 1));
#pragma unroll
      for (int j = 0; j < NJ; ++j) bn[j] = ld4(bp + j * bstride + 16 * (g + 1));
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (SPLIT && (t & 1)) acc2[j] = kf_mfma(f4(a, t), f4(b[j], t), acc2[j]);
        else acc[j] = kf_mfma(f4(a, t), f4(b[j], t), acc[j]);
      }
    a = an;
#pragma unroll
    for (int j = 0; j < NJ; ++j) b[j] = bn[j];
  }
  if constexpr (SPLIT) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] += acc2[j];
  }
}

// the same with a run-time count of B column tiles (0 .. NA)
template <int NA>
__device__ __forceinline__ void kf_mfma_groups_n(int nj, const float* ap, const float* bp, int bstride, int ng,
                                                 f32x4 (&acc)[NA]) {
  switch (nj) {
#define KF_CASE(n)                                                      \
  case n:                                                               \
    if constexpr (n <= NA) kf_mfma_groups<n>(ap, bp, bstride, ng, acc); \
    break;
    KF_CASE(9) KF_CASE(8) KF_CASE(7) KF_CASE(6) KF_CASE(5) KF_CASE(4) KF_CASE(3) KF_CASE(2) KF_CASE(1)
#undef KF_CASE
    default: break;
  }
}

// The two sets stay translation units of their own: with both in one unit the compiler scheduled
// kan_dw_fused_kernel differently (152 instead of 156 VGPRs), and the grid-5 kernels are to stay
// instruction for instruction what they were.
// where the head pass takes g from (kan_head_train_kernel)
enum { KAN_HEAD_MSE = 0, KAN_HEAD_L1 = 1, KAN_HEAD_GIVEN = 2 };

// The head's training pass, what both sets' kernels share of a row (they differ in where a lane's
// weights and weight-gradient sums live).  The row's g, its output o as stored, and the wave's loss
// sum: g is read (KAN_HEAD_GIVEN: yc is g), or it is the loss gradient against the target yc, with
// the row's loss term added to sse (valid: row < n_valid; the others contribute nothing).  By
// value: with reference parameters, and with the kernels' x / y prefetch and out / g stores as
// helpers too, the compiler allocated registers or merged waits differently in the grid-5 kernels.
struct KanHeadG {
  float gn, sse, o;
};
template <int SRC>
__device__ __forceinline__ KanHeadG kan_head_g(float v, float yc, bool valid, float gfac, float sse) {
  float gn = 0.f, o = 0.f;
  if constexpr (SRC == KAN_HEAD_GIVEN) {
    gn = yc;
  } else {
    o = (0.f + v) + 0.f;  // head_loss's accumulation of the one partial and the zero bias
    if (valid) {
      const float err = o - yc;
      if constexpr (SRC == KAN_HEAD_L1) {
        sse += fabsf(err);
        gn = (err > 0.f ? 1.0f : (err < 0.f ? -1.0f : 0.f)) * gfac;
      } else {
        sse += err * err;
        gn = err * gfac;
      }
    }
  }
  return KanHeadG{gn, sse, o};
}

// the block's loss partial: the four waves' sums in wave order (after the barrier that follows the
// waves' sse_w[wv] = sse)
__device__ __forceinline__ float kan_head_sse(const float* sse_w) {
  return ((sse_w[0] + sse_w[1]) + sse_w[2]) + sse_w[3];
}

// out[e] = sum_z slab[z][e] in a fixed order: a block takes C columns; its 256 / C thread groups
// sum every (256/C)-th slab row (4 loads in flight per thread), then the group partials add up
// in group order.  C = 64 for wide slabs; C = 16 (64-byte row segments, 16 groups) when there are
// few columns and many slab rows.
template <int C>
__global__ __launch_bounds__(256) void kan_slab_reduce_kernel(const float* __restrict__ slab, int splits, int64_t mn,
                                                              float* __restrict__ out) {
  constexpr int NG = 256 / C;
  __shared__ float part[NG][C];
  const int col = threadIdx.x % C, grp = threadIdx.x / C;
  const int64_t e = (int64_t)blockIdx.x * C + col;
  float acc = 0.f;
  if (e < mn) {
    int z = grp;
    for (; z + 3 * NG < splits; z += 4 * NG) {
      const float a0 = slab[(int64_t)z * mn + e], a1 = slab[(int64_t)(z + NG) * mn + e];
      const float a2 = slab[(int64_t)(z + 2 * NG) * mn + e], a3 = slab[(int64_t)(z + 3 * NG) * mn + e];
      acc = (((acc + a0) + a1) + a2) + a3;
    }
    for (; z < splits; z += NG) acc += slab[(int64_t)z * mn + e];
  }
  part[grp][col] = acc;
  __syncthreads();
  if (grp == 0 && e < mn) {
    float v = part[0][col];
#pragma unroll
    for (int g = 1; g < NG; ++g) v += part[g][col];
    out[e] = v;
  }
}

static hipError_t slab_reduce(const float* slab, int splits, int64_t mn, float* out, hipStream_t s) {
  if (mn < 64 * 256 && splits > 64)
    hipLaunchKernelGGL(kan_slab_reduce_kernel<16>, dim3((unsigned)((mn + 15) / 16)), dim3(256), 0, s, slab, splits, mn, out);
  else
    hipLaunchKernelGGL(kan_slab_reduce_kernel<64>, dim3((unsigned)((mn + 63) / 64)), dim3(256), 0, s, slab, splits, mn, out);
  return hipGetLastError();
}

static inline int ew_grid(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

// Row splits of a split-K backward kernel with `per` chunk tiles: one round of `resident` blocks
// (every CU busy, no tail), at most max_splits, each a multiple of 64 rows; the grid pads the
// splits to a multiple of 8 (kf_split_block).  blocks = 0: too many for a 1-D grid.
struct KfSplitPlan {
  int64_t rows_per_split;
  int z;            // splits that hold rows = slabs written
  unsigned blocks;
};
static KfSplitPlan kf_plan_splits(int64_t N, int64_t resident, int64_t per, int64_t max_splits) {
  int64_t splits = resident / per;
  if (splits < 1) splits = 1;
  if (splits > max_splits) splits = max_splits;
  int64_t rps = (N + splits - 1) / splits;
  rps = (rps + KF_R - 1) / KF_R * KF_R;
  const int z = (int)((N + rps - 1) / rps);
  const int64_t blocks = per * ((z + 7) / 8 * 8);
  return KfSplitPlan{rps, z, blocks > 0x7fffffff ? 0u : (unsigned)blocks};
}

// The weight-gradient pass's grid: chunk tiles of ic inputs x 64 outs, split over the rows in one
// resident round.  split.blocks = 0: too many for a 1-D grid.
struct KfDwPlan {
  int nchunk, nout;
  KfSplitPlan split;
};
static KfDwPlan kf_plan_dw(int64_t N, int in, int out, int ic, int64_t max_splits) {
  const int nchunk = (in + ic - 1) / ic, nout = (out + KF_O - 1) / KF_O;
  return KfDwPlan{nchunk, nout, kf_plan_splits(N, kKanResidentBlocks, (int64_t)nchunk * nout, max_splits)};
}

// The head pass's blocks: >= 256 contiguous rows each, at most `slots` (slab rows) and max_parts
// (loss partials) of them.  One partition for both kernel sets and the three sources of g, so a
// given g reproduces the pass that wrote it bit for bit.
struct KanHeadPlan {
  int64_t rows_per_block;
  unsigned blocks;
};
static KanHeadPlan kan_head_plan(int64_t N, int64_t slots, int64_t max_parts) {
  int64_t blocks = (N + 255) / 256;
  if (blocks > slots) blocks = slots;
  if (blocks > max_parts) blocks = max_parts;
  const int64_t rpb = (N + blocks - 1) / blocks;
  return KanHeadPlan{rpb, (unsigned)((N + rpb - 1) / rpb)};
}

// ---- the grid-5 launchers of kan.hip, called by the entry points in kan_general.hip (which have
// checked the shapes) ----------------------------------------------------------------------------
hipError_t kan5_fwd_fused(const float* X, const float* grid, const float* W, int64_t N, int in, int out, float* Y,
                          hipStream_t s);
hipError_t kan5_head_fwd(const float* X, const float* grid, const float* W, int64_t N, int in, float* Y, hipStream_t s);
hipError_t kan5_head_pass(int src, const KanHeadPlan& p, const float* X, const float* grid, const float* W,
                          const float* yg, int64_t N, int in, int64_t n_valid, float gfac, float* out, float* g,
                          float* sse_part, float* slab, float* Gin, hipStream_t s);
hipError_t kan5_dw_fused(const KfDwPlan& p, const float* X, const float* grid, const float* G, int64_t N, int in,
                         int out, float* slab, hipStream_t s);
hipError_t kan5_dx_fused(const float* X, const float* grid, const float* Gout, const float* WT, int64_t N, int in,
                         int out, float* Gin, hipStream_t s);
hipError_t kan5_bwd_fused(const float* X, const float* grid, const float* G, const float* WT, int64_t N, int in,
                          int out, int64_t max_splits, float* slab, float* dW, float* Gin, hipStream_t s);

}  // namespace siren
