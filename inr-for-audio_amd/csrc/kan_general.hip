// KAN kernels for any grid size (kan.py KANLinear(grid_size=G), spline_order 3): the twins of kan.hip's
// grid-5 kernels with G as a launch argument.  kan.hip supplies the basis division, the tile
// loaders, the MFMA loop, the split plan and the slab reduction (its part above KAN_TILES_ONLY).
#define KAN_TILES_ONLY
#include "kan.hip"

namespace siren {

// ---- any grid size (spline_order 3, 1 <= grid_size <= KG_MAX_GRID) ------------------------------
// A second kernel set with the grid size G as a launch argument: NB = G + 3 bases, NG = G + 7 knots
// and K1 = G + 4 A-columns per input are run-time values, one code object per kernel.  grid_size 5
// keeps kan.hip's kernels; these run every other size (and 5 under SIREN_OPT_KAN_GENERAL).
// What a (row, input) pair costs does not grow with G: one span s, four non-zero bases B[s-3 .. s]
// (kg_bases_window: the recursion of kan_bases_window on run-time table strides, the span found by
// bisection instead of a count over the knots).  The pair's thread keeps that window and never
// b[NB]: it writes the four values into a zero-filled A tile at columns ic + NB ii + (s - 3 + q),
// and the dA tile is read back the same way.  The LDS tiles and the MFMA loop are kan.hip's;
// a chunk takes IC = min(16, 144 / K1) inputs so that its K1 IC columns fit the 144-column tiles
// (G = 5: 16 inputs, G = 11: 9, G = 64: 2).  The backward always runs as kang_dw_fused +
// kang_dx_fused (no one-pass twin of kan_bwd_fused).
// The skipped columns of a row hold exact zeros in kan.hip's kernels too, where they enter the
// k-ordered sums as +-0 terms, so at G = 5 both sets add the same non-zero terms in the same order.
struct KgDims {
  int nb, ng, k1, ic;  // bases, knots, A-columns per input; inputs per chunk
  int gst, vst;        // LDS strides (odd) of an input's knot row and of its 3 (NG - 1) reciprocals
};
__host__ __device__ constexpr KgDims kg_dims(int G) {
  return KgDims{G + 3, G + 7, G + 4, KF_KC / (G + 4) < KF_IC ? KF_KC / (G + 4) : KF_IC, (G + 7) | 1, (3 * (G + 6)) | 1};
}
// a chunk's knot rows and reciprocal tables: ic gst <= ic (K1 + 4) <= 144 + 64 and
// ic vst <= ic (3 K1 + 7) <= 432 + 112 floats
constexpr int KG_GK = 208, KG_INV = 544;
constexpr bool kg_tables_fit() {
  for (int G = 1; G <= KG_MAX_GRID; ++G) {
    const KgDims d = kg_dims(G);
    if (d.ic < 1 || d.k1 * d.ic > KF_KC || d.ic * d.gst > KG_GK || d.ic * d.vst > KG_INV) return false;
  }
  return true;
}
static_assert(kg_tables_fit(), "a chunk's columns, knots or reciprocals outgrow their LDS arrays");

struct KgChunk {
  int i0, ic, kc, kpad, nkt, nb;  // KfChunk's fields, and the bases per input
  __device__ __forceinline__ int col(int kk, int in) const { return kk < ic ? i0 + kk : in + nb * i0 + (kk - ic); }
};
__device__ __forceinline__ KgChunk kg_chunk(int i0, int in, const KgDims& d) {
  const int ic = in - i0 < d.ic ? in - i0 : d.ic, kc = d.k1 * ic, kpad = (kc + 15) & ~15;
  return KgChunk{i0, ic, kc, kpad, kpad >> 4, d.nb};
}

// kan_bases_window for ng knots: s (-1 outside the grid), w[q] = B[s-3+q] and, with DERIV,
// d[q] = B'[s-3+q].  The same operations in the same order, so the same bits; inv is the input's
// table inv[(k-1)(ng-1) + j] = RN(1 / (g[j+k] - g[j])) (kg_fill_inv).  The span: for non-decreasing
// knots #{j : g[j] <= x} is where the predicate x >= g[j] turns false, found by bisection (a NaN
// fails every comparison: count 0, no span).  Slots whose basis index s-3+q falls outside 0 .. NB-1
// hold values of discarded terms: the callers skip them.
template <bool DERIV, bool RCP>
__device__ __forceinline__ int kg_bases_window(float x, const float* __restrict__ g, int ng, float* w, float* d,
                                               const float* __restrict__ inv) {
  int lo = 0, hi = ng;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x >= g[mid]) lo = mid + 1;
    else hi = mid;
  }
  const int s = (lo >= 1 && lo <= ng - 1) ? lo - 1 : -1;
  const int s0 = s < 0 ? 0 : s;
  float kw[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    int t = s0 - 3 + e;
    t = t < 0 ? 0 : (t > ng - 1 ? ng - 1 : t);
    kw[e] = g[t];
  }
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

// gk[ii * gst + j] = knot j of input i0 + ii;  inv[ii * vst + (k-1)(ng-1) + j] = RN(1 / (g[j+k] - g[j]))
__device__ __forceinline__ void kg_fill_knots(float* gk, const float* __restrict__ grid, int i0, int ic, const KgDims& d) {
  for (int e = threadIdx.x; e < ic * d.ng; e += blockDim.x) {
    const int ii = e / d.ng;
    gk[ii * d.gst + (e - ii * d.ng)] = grid[(int64_t)i0 * d.ng + e];
  }
}
__device__ __forceinline__ void kg_fill_inv(float* inv, const float* __restrict__ grid, int i0, int ic, const KgDims& d) {
  const int n1 = d.ng - 1, per = 3 * n1;
  for (int e = threadIdx.x; e < ic * per; e += blockDim.x) {
    const int ii = e / per, q = e - ii * per, k = q / n1 + 1, j = q - (k - 1) * n1;
    const float* g = grid + (int64_t)(i0 + ii) * d.ng;
    inv[ii * d.vst + q] = (j + k < d.ng) ? 1.0f / (g[j + k] - g[j]) : 0.0f;
  }
}

// Y[n][o] = sum_k A[n][k] W[o][k] as kan_fwd_fused_kernel: grid (ceil(N/64), ceil(out/64)), wave w
// rows 16w .. 16w+15 x 64 outs.  Per chunk the A tile is zero-filled while W, the knots and the
// reciprocals load; after the barrier each (row, input) pair writes SiLU(x) and its four bases.
__global__ __launch_bounds__(256) void kang_fwd_fused_kernel(const float* __restrict__ X, const float* __restrict__ grid,
                                                             const float* __restrict__ W, int64_t N, int in, int out,
                                                             int G, float* __restrict__ Y) {
  __shared__ __attribute__((aligned(16))) float As[KF_R][KF_AST];  // [row][kk]
  __shared__ __attribute__((aligned(16))) float Ws[KF_O][KF_AST];  // [o][kk]
  __shared__ float gk[KG_GK];
  __shared__ float inv[KG_INV];
  const KgDims d = kg_dims(G);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * KF_R;
  const int o0 = blockIdx.y * KF_O;
  const int64_t K = (int64_t)d.k1 * in;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i0 = 0; i0 < in; i0 += d.ic) {
    const KgChunk ch = kg_chunk(i0, in, d);
    const int kpad = ch.kpad, k4 = kpad >> 2;
    kg_fill_knots(gk, grid, i0, ch.ic, d);
    kg_fill_inv(inv, grid, i0, ch.ic, d);
    for (int e = tid; e < KF_O * kpad; e += 256) {
      const int o = e / kpad, kk = e - o * kpad;
      Ws[o][kk] = (o0 + o < out && kk < ch.kc) ? W[(int64_t)(o0 + o) * K + ch.col(kk, in)] : 0.f;
    }
    for (int e = tid; e < KF_R * k4; e += 256) {
      const int r = e / k4, c4 = e - r * k4;
      *reinterpret_cast<float4*>(&As[r][4 * c4]) = float4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    for (int p = tid; p < KF_R * ch.ic; p += 256) {
      const int r = p & (KF_R - 1), ii = p >> 6;
      if (r0 + r >= N) continue;
      const float x = X[(r0 + r) * in + i0 + ii];
      float w[4], unused[4];
      const int s = kg_bases_window<false, false>(x, gk + ii * d.gst, d.ng, w, unused, inv + ii * d.vst);
      As[r][ii] = silu(x);
      if (s < 0) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = s - 3 + q;
        if (c >= 0 && c < d.nb) As[r][ch.ic + d.nb * ii + c] = w[q];
      }
    }
    __syncthreads();
    kf_mfma_groups<4, 4, false>(&As[16 * wv + li][4 * lk], &Ws[li][4 * lk], 16 * KF_AST, kpad >> 4, acc);
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t n = r0 + 16 * wv + 4 * lk + q;
      const int o = o0 + 16 * j + li;
      if (n < N && o < out) Y[n * out + o] = acc[j][q];
    }
}

// ---- the last layer at any grid size (out = 1, in <= 64): one wave per row, lane = input -------
// The lane's K1 weights no longer fit registers, and its weight-gradient partials are indexed by the
// row's span, so both live in LDS beside the knots and reciprocals, in dynamic LDS sized by (in, G):
//   gk [in][gst]  inv [in][vst]  wl [in][wst]: lane i's W[i], W[in + NB i + c]   (odd strides:
//   lane-consecutive rows fall on distinct banks), and for the training pass
//   part [4 waves][K1][64]: column t of lane i's input, owned by that lane of that wave, which
//   adds its rows' terms in program order (lane-consecutive: conflict-free whatever the spans),
//   and the four waves' loss partials.
// At in = 64, G = 64: 18 176 + 54 016 + 17 664 B, + 69 648 B of partials = 159 504 B of the CU's
// 163 840 (one block per CU there; at G = 20 it is 58 KB).
struct KgHead {
  const float *gk, *inv, *wl;
  float* part;
  int wst;
};
__host__ __device__ inline int kg_head_wst(const KgDims& d) { return d.k1 | 1; }
static size_t kg_head_lds_bytes(int in, int G, bool train) {
  const KgDims d = kg_dims(G);
  return sizeof(float) * ((size_t)in * (d.gst + d.vst + kg_head_wst(d)) + (train ? 4 * d.k1 * 64 + 4 : 0));
}

__device__ __forceinline__ KgHead kg_head_setup(float* smem, const float* __restrict__ grid, const float* __restrict__ W,
                                                int in, const KgDims& d) {
  float* gk = smem;
  float* inv = gk + in * d.gst;
  float* wl = inv + in * d.vst;
  const int wst = kg_head_wst(d);
  kg_fill_knots(gk, grid, 0, in, d);
  kg_fill_inv(inv, grid, 0, in, d);
  for (int e = threadIdx.x; e < in * d.k1; e += blockDim.x) {
    const int i = e / d.k1, t = e - i * d.k1;
    wl[i * wst + t] = t == 0 ? W[i] : W[in + d.nb * i + (t - 1)];
  }
  return KgHead{gk, inv, wl, wl + in * wst, wst};
}

// kan_head_row on the window: the row's output on every lane; on the lanes with an input also
// sl = SiLU(x), dsl = SiLU'(x) (DERIV), the span s and the window w[] = B, dw[] = B' (DERIV) with
// the slots outside 0 .. NB-1 (and all of them without a span) zeroed
template <bool DERIV>
__device__ __forceinline__ float kg_head_row(bool on, float x, int lane, const KgHead& h, const KgDims& d, float& sl,
                                             float& dsl, int& s, float* w, float* dw) {
  float v = 0.f;
  s = -1;
  if (on) {
    s = kg_bases_window<DERIV, false>(x, h.gk + lane * d.gst, d.ng, w, dw, h.inv + lane * d.vst);
    if constexpr (DERIV) silu_and_grad(x, sl, dsl);
    else sl = silu(x);
    const float* wl = h.wl + lane * h.wst;
    v = sl * wl[0];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = s - 3 + q;
      if (s >= 0 && c >= 0 && c < d.nb) {
        v += w[q] * wl[1 + c];
      } else {
        w[q] = 0.f;
        if constexpr (DERIV) dw[q] = 0.f;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void kang_head_fwd_kernel(const float* __restrict__ X, const float* __restrict__ grid,
                                                            const float* __restrict__ W, int64_t N, int in, int G,
                                                            float* __restrict__ Y) {
  extern __shared__ __attribute__((aligned(16))) float kg_smem[];
  const KgDims d = kg_dims(G);
  const KgHead h = kg_head_setup(kg_smem, grid, W, in, d);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const bool on = lane < in;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t n = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); n < N; n += nw) {
    float sl, unused, w[4], dw[4];
    int s;
    const float v = kg_head_row<false>(on, on ? X[n * in + lane] : 0.f, lane, h, d, sl, unused, s, w, dw);
    if (lane == 0) Y[n] = v;
  }
}

// kan_head_train_kernel at any grid size: the same block partition, row order and sources of g.
// The spline partials go to the wave's LDS columns (kg_head_setup) instead of registers.
template <int SRC>
__global__ __launch_bounds__(256) void kang_head_train_kernel(const float* __restrict__ X, const float* __restrict__ grid,
                                                              const float* __restrict__ W, const float* __restrict__ yg,
                                                              int64_t N, int in, int G, int64_t n_valid, float gfac,
                                                              int64_t rows_per_block, float* __restrict__ out,
                                                              float* __restrict__ g, float* __restrict__ sse_part,
                                                              float* __restrict__ slab, float* __restrict__ Gin) {
  constexpr bool GIVEN = SRC == KAN_HEAD_GIVEN;
  extern __shared__ __attribute__((aligned(16))) float kg_smem[];
  const KgDims d = kg_dims(G);
  const KgHead h = kg_head_setup(kg_smem, grid, W, in, d);
  float* sse_w = h.part + 4 * d.k1 * 64;  // the waves' loss partials, after theirs of the weights
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* part = h.part + (wv * d.k1) * 64 + lane;  // part[wv][t][lane] = part[t * 64]
  for (int t = 0; t < d.k1; ++t) part[t * 64] = 0.f;
  __syncthreads();
  const int64_t nb = (int64_t)blockIdx.x * rows_per_block;
  const int64_t ne = nb + rows_per_block < N ? nb + rows_per_block : N;
  const int64_t nyg = GIVEN ? ne : n_valid;  // rows whose yg is read: a given g covers the pad rows
  const bool on = lane < in;
  const float* wl = h.wl + lane * h.wst;
  float ab = 0.f, sse = 0.f;
  int64_t n = nb + wv;
  float xn = 0.f, yn = 0.f;
  if (n < ne) {
    if (on) xn = X[n * in + lane];
    if (n < nyg) yn = yg[n];
  }
  for (; n < ne; n += 4) {
    const float xc = xn, yc = yn;
    if (n + 4 < ne) {
      if (on) xn = X[(n + 4) * in + lane];
      if (n + 4 < nyg) yn = yg[n + 4];
    }
    float sl = 0.f, dsl = 0.f, w[4], dw[4];
    int s;
    const float v = kg_head_row<true>(on, xc, lane, h, d, sl, dsl, s, w, dw);
    float gn = 0.f;
    if constexpr (GIVEN) {
      gn = yc;
    } else {
      const float o = (0.f + v) + 0.f;  // head_loss's accumulation of the one partial and the zero bias
      if (n < n_valid) {
        const float err = o - yc;
        if constexpr (SRC == KAN_HEAD_L1) {
          sse += fabsf(err);
          gn = (err > 0.f ? 1.0f : (err < 0.f ? -1.0f : 0.f)) * gfac;
        } else {
          sse += err * err;
          gn = err * gfac;
        }
      }
      if (lane == 0) {
        out[n] = o;
        g[n] = gn;
      }
    }
    if (on) {
      ab += gn * sl;
      float dx = dsl * wl[0];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = s - 3 + q;
        if (s >= 0 && c >= 0 && c < d.nb) {
          part[(1 + c) * 64] += gn * w[q];
          dx += dw[q] * wl[1 + c];
        }
      }
      Gin[n * in + lane] = gn * dx;
    }
  }
  part[0] = ab;
  if (!GIVEN && lane == 0) sse_w[wv] = sse;
  __syncthreads();
  if (wv == 0) {
    if (on) {
      float* row = slab + (int64_t)blockIdx.x * d.k1 * in;
      const float* p = h.part + lane;
      const int ws = d.k1 * 64;
      for (int t = 0; t < d.k1; ++t) {
        const float v = ((p[t * 64] + p[ws + t * 64]) + p[2 * ws + t * 64]) + p[3 * ws + t * 64];
        row[t == 0 ? lane : in + d.nb * lane + (t - 1)] = v;
      }
    }
    if (!GIVEN && lane == 0) sse_part[blockIdx.x] = ((sse_w[0] + sse_w[1]) + sse_w[2]) + sse_w[3];
  }
}

// ---- the split backward at any grid size -----------------------------------------------------
// As[kk][r] (stride KF_CST): the chunk's A columns for rows r0 + r.  The caller zero-fills the tile
// (kg_zero_a) before the barrier that precedes this call; each pair then writes its five values
// (v_rcp_f32 quotients, as kf_fill_a).
__device__ __forceinline__ void kg_zero_a(float (*As)[KF_CST], const KgChunk& ch) {
  for (int e = threadIdx.x; e < ch.kpad * (KF_R / 4); e += blockDim.x)
    *reinterpret_cast<float4*>(&As[e >> 4][4 * (e & 15)]) = float4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void kg_fill_a(float (*As)[KF_CST], const float (*Xs)[KF_IC + 1], const float* gk, int64_t re,
                                          int64_t r0, const KgChunk& ch, const KgDims& d) {
  for (int p = threadIdx.x; p < KF_R * ch.ic; p += blockDim.x) {
    const int r = p & (KF_R - 1), ii = p >> 6;
    if (r0 + r >= re) continue;
    const float x = Xs[r][ii];
    float w[4], unused[4];
    const int s = kg_bases_window<false, true>(x, gk + ii * d.gst, d.ng, w, unused, nullptr);
    As[ii][r] = silu(x);
    if (s < 0) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = s - 3 + q;
      if (c >= 0 && c < d.nb) As[ch.ic + d.nb * ii + c][r] = w[q];
    }
  }
}

// kf_store_slab on a KgChunk: slab[z][o + q][col(kk)] = acc[j][q]
template <int NA>
__device__ __forceinline__ void kg_store_slab(float* __restrict__ slab, int z, const f32x4 (&acc)[NA], int nj, int kk0,
                                              int o, const KgChunk& ch, int in, int out, int k1) {
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

// kan_dw_fused_kernel at any grid size: the same grid, splits and wave tiling
__global__ __launch_bounds__(256) void kang_dw_fused_kernel(const float* __restrict__ X, const float* __restrict__ grid,
                                                            const float* __restrict__ Gr, int64_t N, int in, int out,
                                                            int G, int64_t rows_per_split, int nchunk, int nout,
                                                            int splits, float* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) float As[KF_KC][KF_CST];  // [kk][r]
  __shared__ __attribute__((aligned(16))) float Gt[KF_O][KF_CST];   // [o][r]
  __shared__ float Xs[KF_R][KF_IC + 1];
  __shared__ float gk[KG_GK];
  int cid, z;
  kf_split_block(nchunk * nout, cid, z);
  if (z >= splits) return;  // whole block, before any barrier
  const KgDims d = kg_dims(G);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const int o0 = (cid / nchunk) * KF_O;
  const KgChunk ch = kg_chunk((cid % nchunk) * d.ic, in, d);
  kg_fill_knots(gk, grid, ch.i0, ch.ic, d);
  const int64_t rb = (int64_t)z * rows_per_split;
  const int64_t re = rb + rows_per_split < N ? rb + rows_per_split : N;
  f32x4 acc[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t r0 = rb; r0 < re; r0 += KF_R) {
    kf_stage_x(Xs, X, re, in, r0, ch.i0, ch.ic);
    if ((out & 3) == 0 && o0 + KF_O <= out) {
      KfGRegs<256> v;
      kf_g_load<256, true>(v, Gr, re, out, r0, o0);
      kf_g_store<256, true, true>(&Gt[0][0], v);
    } else {
      kf_g_scalar<256, false, true>(&Gt[0][0], Gr, re, out, r0, o0);
    }
    kg_zero_a(As, ch);
    __syncthreads();
    kg_fill_a(As, Xs, gk, re, r0, ch, d);
    __syncthreads();
    kf_mfma_groups_n(ch.nkt, &Gt[16 * wv + li][4 * lk], &As[li][4 * lk], 16 * KF_CST, KF_R / 16, acc);
    __syncthreads();
  }
  kg_store_slab(slab, z, acc, ch.nkt, li, o0 + 16 * wv + 4 * lk, ch, in, out, d.k1);
}

// kan_dx_fused_kernel at any grid size.  The pair's contraction reads its window of the dA row:
//   Gin[n][i] = SiLU'(x) dA[n][i] + sum_q B'[s-3+q](x) dA[n][in + NB i + (s-3+q)]
__global__ __launch_bounds__(256) void kang_dx_fused_kernel(const float* __restrict__ X, const float* __restrict__ grid,
                                                            const float* __restrict__ Gout, const float* __restrict__ WT,
                                                            int64_t N, int in, int out, int G, float* __restrict__ Gin) {
  __shared__ __attribute__((aligned(16))) float Gs[KF_R][KF_CST];   // [r][o]
  __shared__ __attribute__((aligned(16))) float WD[KF_KC * KF_CST];  // Wt[kk][o], then dAs[r][kk]
  __shared__ float Xs[KF_R][KF_IC + 1];
  __shared__ float gk[KG_GK];
  const KgDims d = kg_dims(G);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * KF_R;
  const bool g_once = out <= KF_O;
  for (int i0 = 0; i0 < in; i0 += d.ic) {
    const KgChunk ch = kg_chunk(i0, in, d);
    f32x4 acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    kg_fill_knots(gk, grid, i0, ch.ic, d);
    kf_stage_x(Xs, X, N, in, r0, i0, ch.ic);
    for (int oc = 0; oc < out; oc += KF_O) {
      const int on = out - oc < KF_O ? out - oc : KF_O, opad = (on + 15) & ~15;
      if (!g_once || i0 == 0) {
        if ((out & 3) == 0 && on == KF_O) {
          KfGRegs<256> v;
          kf_g_load<256, false>(v, Gout, N, out, r0, oc);
          kf_g_store<256, false, false>(&Gs[0][0], v);
        } else {
          kf_g_scalar<256, false, false>(&Gs[0][0], Gout, N, out, r0, oc);
        }
      }
      // Wt[kk][o] = W[oc + o][col(kk)] from the transposed copy; rows past kc and outs past `out` zero
      for (int e = tid; e < ch.kpad * KF_O; e += 256) {
        const int kk = e / KF_O, o = e % KF_O;
        WD[kk * KF_CST + o] = (kk < ch.kc && oc + o < out) ? WT[(int64_t)ch.col(kk, in) * out + oc + o] : 0.f;
      }
      __syncthreads();
      kf_mfma_groups_n(ch.nkt, &Gs[16 * wv + li][4 * lk], &WD[li * KF_CST + 4 * lk], 16 * KF_CST, opad >> 4, acc);
      __syncthreads();
    }
    // dA -> LDS over the W chunk, then each pair contracts its window (kf_da_to_gin's steps)
#pragma unroll
    for (int j = 0; j < 9; ++j)
      if (j < ch.nkt)
#pragma unroll
        for (int q = 0; q < 4; ++q) WD[(16 * wv + 4 * lk + q) * KF_DST + li + 16 * j] = acc[j][q];
    __syncthreads();
    for (int p = tid; p < KF_R * ch.ic; p += 256) {
      const int r = p & (KF_R - 1), ii = p >> 6;
      if (r0 + r >= N) continue;
      const float x = Xs[r][ii];
      float w[4], dw[4], sl, ds;
      const int s = kg_bases_window<true, true>(x, gk + ii * d.gst, d.ng, w, dw, nullptr);
      silu_and_grad(x, sl, ds);
      const float* dA = WD + r * KF_DST;
      float v = ds * dA[ii];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = s - 3 + q;
        if (s >= 0 && c >= 0 && c < d.nb) v += dw[q] * dA[ch.ic + d.nb * ii + c];
      }
      Xs[r][ii] = v;
    }
    __syncthreads();
    for (int e = tid; e < KF_R * ch.ic; e += 256) {
      const int r = e / ch.ic, ii = e - r * ch.ic;
      if (r0 + r < N) Gin[(r0 + r) * in + ch.i0 + ii] = Xs[r][ii];
    }
    __syncthreads();  // Xs / gk / WD are refilled by the next chunk
  }
}

// kan_combine / kan_param_grads with nb bases per input (k1 = nb + 1 columns)
__global__ void kang_combine_kernel(const float* __restrict__ base_w, const float* __restrict__ spline_w,
                                    const float* __restrict__ scaler, int out, int in, int nb, float* __restrict__ W,
                                    float* __restrict__ WT) {
  const int total = out * in;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int o = e / in, i = e - o * in;
    float* row = W + (int64_t)o * (nb + 1) * in;
    row[i] = base_w[e];
    if (WT) WT[(int64_t)i * out + o] = base_w[e];
    const float s = scaler[e];
    for (int c = 0; c < nb; ++c) {
      const float v = spline_w[(int64_t)e * nb + c] * s;
      row[in + nb * i + c] = v;
      if (WT) WT[(int64_t)(in + nb * i + c) * out + o] = v;
    }
  }
}

__global__ void kang_param_grads_kernel(const float* __restrict__ dW, const float* __restrict__ spline_w,
                                        const float* __restrict__ scaler, int out, int in, int nb, int accumulate,
                                        float* __restrict__ g_base, float* __restrict__ g_spline,
                                        float* __restrict__ g_scaler) {
  const int total = out * in;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int o = e / in, i = e - o * in;
    const float* row = dW + (int64_t)o * (nb + 1) * in;
    const float s = scaler[e];
    float gs = 0.f;
    for (int c = 0; c < nb; ++c) {
      const float dv = row[in + nb * i + c];
      const int64_t k = (int64_t)e * nb + c;
      const float v = dv * s;
      g_spline[k] = accumulate ? g_spline[k] + v : v;
      gs += dv * spline_w[k];
    }
    g_base[e] = accumulate ? g_base[e] + row[i] : row[i];
    g_scaler[e] = accumulate ? g_scaler[e] + gs : gs;
  }
}

static bool kg_grid_ok(int G) { return G >= 1 && G <= KG_MAX_GRID; }

// The head kernels' dynamic LDS can pass the 64 KB a kernel gets by default: the first launch that
// needs more raises the kernel's limit to the CU's 160 KB, once (these kernels have no static LDS).
// Not a stream operation, so a launch under graph capture may be that first one.
constexpr size_t kKgHeadLdsMax = 160 * 1024;
template <class Kern>
static hipError_t kg_head_lds(Kern kernel, size_t bytes, bool& raised) {  // raised: the caller's flag of this kernel
  if (bytes <= 64 * 1024 || raised) return bytes <= kKgHeadLdsMax ? hipSuccess : hipErrorInvalidValue;
  if (bytes > kKgHeadLdsMax) return hipErrorInvalidValue;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kKgHeadLdsMax);
  raised = e == hipSuccess;
  return e;
}

hipError_t kang_fwd_fused(const float* X, const float* grid, const float* W, int64_t N, int in, int out, int G, float* Y,
                          hipStream_t s) {
  if (N <= 0 || in <= 0 || out <= 0 || !kg_grid_ok(G)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kang_fwd_fused_kernel, dim3((unsigned)((N + KF_R - 1) / KF_R), (out + KF_O - 1) / KF_O), dim3(256),
                     0, s, X, grid, W, N, in, out, G, Y);
  return hipGetLastError();
}

hipError_t kang_head_fwd(const float* X, const float* grid, const float* W, int64_t N, int in, int G, float* Y,
                         hipStream_t s) {
  if (N <= 0 || in <= 0 || in > 64 || !kg_grid_ok(G)) return hipErrorInvalidValue;
  const size_t lds = kg_head_lds_bytes(in, G, false);
  static bool raised = false;
  const hipError_t e = kg_head_lds(kang_head_fwd_kernel, lds, raised);
  if (e != hipSuccess) return e;
  const int64_t blocks = (N + 3) / 4;
  hipLaunchKernelGGL(kang_head_fwd_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), lds, s, X, grid,
                     W, N, in, G, Y);
  return hipGetLastError();
}

// kan_head_pass at any grid size: the same block partition
template <int SRC>
static hipError_t kang_head_pass(const float* X, const float* grid, const float* W, const float* yg, int64_t N, int in,
                                 int G, int64_t n_valid, float gfac, int64_t slots, int64_t max_parts, float* out,
                                 float* g, float* sse_part, float* slab, float* dW, float* Gin, int* nparts,
                                 hipStream_t s) {
  if (N <= 0 || in <= 0 || in > 64 || slots < 1 || max_parts < 1 || !kg_grid_ok(G)) return hipErrorInvalidValue;
  const size_t lds = kg_head_lds_bytes(in, G, true);
  static bool raised = false;  // one per SRC
  const hipError_t e = kg_head_lds(kang_head_train_kernel<SRC>, lds, raised);
  if (e != hipSuccess) return e;
  int64_t blocks = (N + 255) / 256;
  if (blocks > slots) blocks = slots;
  if (blocks > max_parts) blocks = max_parts;
  const int64_t rpb = (N + blocks - 1) / blocks;
  blocks = (N + rpb - 1) / rpb;
  hipLaunchKernelGGL(kang_head_train_kernel<SRC>, dim3((unsigned)blocks), dim3(256), lds, s, X, grid, W, yg, N, in, G,
                     n_valid, gfac, rpb, out, g, sse_part, slab, Gin);
  if (nparts) *nparts = (int)blocks;
  return slab_reduce(slab, (int)blocks, (int64_t)kg_dims(G).k1 * in, dW, s);
}

hipError_t kang_head_train(const float* X, const float* grid, const float* W, const float* y, int64_t N, int in, int G,
                           int64_t n_valid, float gfac, int64_t slots, int64_t max_parts, float* out, float* g,
                           float* sse_part, float* slab, float* dW, float* Gin, int* nparts, hipStream_t s,
                           int loss_mode) {
  if (!nparts || (loss_mode != 0 && loss_mode != 1)) return hipErrorInvalidValue;
  return loss_mode == 1 ? kang_head_pass<KAN_HEAD_L1>(X, grid, W, y, N, in, G, n_valid, gfac, slots, max_parts, out, g,
                                                      sse_part, slab, dW, Gin, nparts, s)
                        : kang_head_pass<KAN_HEAD_MSE>(X, grid, W, y, N, in, G, n_valid, gfac, slots, max_parts, out, g,
                                                       sse_part, slab, dW, Gin, nparts, s);
}

hipError_t kang_head_bwd(const float* X, const float* grid, const float* W, const float* g, int64_t N, int in, int G,
                         int64_t slots, int64_t max_parts, float* slab, float* dW, float* Gin, hipStream_t s) {
  return kang_head_pass<KAN_HEAD_GIVEN>(X, grid, W, g, N, in, G, N, 0.f, slots, max_parts, nullptr, nullptr, nullptr,
                                        slab, dW, Gin, nullptr, s);
}

hipError_t kang_dw_fused(const float* X, const float* grid, const float* Gr, int64_t N, int in, int out, int G,
                         int64_t max_splits, float* slab, float* dW, hipStream_t s) {
  if (N <= 0 || in <= 0 || out <= 0 || max_splits < 1 || !kg_grid_ok(G)) return hipErrorInvalidValue;
  const KgDims d = kg_dims(G);
  const int nchunk = (in + d.ic - 1) / d.ic, nout = (out + KF_O - 1) / KF_O;
  const KfSplitPlan p = kf_plan_splits(N, kKanResidentBlocks, (int64_t)nchunk * nout, max_splits);
  if (!p.blocks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kang_dw_fused_kernel, dim3(p.blocks), dim3(256), 0, s, X, grid, Gr, N, in, out, G,
                     p.rows_per_split, nchunk, nout, p.z, slab);
  return slab_reduce(slab, p.z, (int64_t)out * d.k1 * in, dW, s);
}

hipError_t kang_dx_fused(const float* X, const float* grid, const float* Gout, const float* WT, int64_t N, int in,
                         int out, int G, float* Gin, hipStream_t s) {
  if (N <= 0 || in <= 0 || out <= 0 || !kg_grid_ok(G)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kang_dx_fused_kernel, dim3((unsigned)((N + KF_R - 1) / KF_R)), dim3(256), 0, s, X, grid, Gout, WT,
                     N, in, out, G, Gin);
  return hipGetLastError();
}

hipError_t kang_combine(const float* base_w, const float* spline_w, const float* scaler, int out, int in, int G,
                        float* W, float* WT, hipStream_t s) {
  if (!kg_grid_ok(G)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kang_combine_kernel, dim3(ew_grid((int64_t)out * in)), dim3(256), 0, s, base_w, spline_w, scaler,
                     out, in, G + 3, W, WT);
  return hipGetLastError();
}

hipError_t kang_param_grads(const float* dW, const float* spline_w, const float* scaler, int out, int in, int G,
                            int accumulate, float* g_base, float* g_spline, float* g_scaler, hipStream_t s) {
  if (!kg_grid_ok(G)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kang_param_grads_kernel, dim3(ew_grid((int64_t)out * in)), dim3(256), 0, s, dW, spline_w, scaler,
                     out, in, G + 3, accumulate, g_base, g_spline, g_scaler);
  return hipGetLastError();
}

}  // namespace siren
