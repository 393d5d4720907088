// KAN kernels for any grid size (kan.py KANLinear(grid_size=G), spline_order 3): the twins of kan.hip's
// grid-5 kernels with G as a launch argument, the refit (kan_regrid_*) for every size, and the one
// family of KAN entry points (siren_kernels.h), which picks the set.  kan_tiles.h supplies the basis
// recursion, the tile loaders, the MFMA loop, the head pass's row steps, the partitions and the slab
// reduction to both sets.
#include "kan_tiles.h"

namespace siren {

// ---- any grid size (spline_order 3, 1 <= grid_size <= KG_MAX_GRID) ------------------------------
// A second kernel set with the grid size G as a launch argument: NB = G + 3 bases, NG = G + 7 knots
// and K1 = G + 4 A-columns per input are run-time values, one code object per kernel.  grid_size 5
// keeps kan.hip's kernels; these run every other size (and 5 under SIREN_OPT_KAN_GENERAL).
// What a (row, input) pair costs does not grow with G: one span s, four non-zero bases B[s-3 .. s]
// (kan_bases_window<.., KAN_SPAN_BISECT>: the one recursion on run-time table strides, the span found
// by bisection instead of a count over the knots).  The pair's thread keeps that window and never
// b[NB]: it writes the four values into a zero-filled A tile at columns ic + NB ii + (s - 3 + q),
// and the dA tile is read back the same way.  The LDS tiles and the MFMA loop are kan_tiles.h's;
// a chunk takes IC = min(16, 144 / K1) inputs so that its K1 IC columns fit the 144-column tiles
// (G = 5: 16 inputs, G = 11: 9, G = 64: 2).  The backward always runs as kang_dw_fused +
// kang_dx_fused (no one-pass twin of kan_bwd_fused: kan_hidden_bwd).
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

// (Not KfChunk with an nb field: filled with the literal 8 it did not fold away in kan_dx_fused_kernel
// and kan_bwd_fused_kernel, which then compiled to other instructions.)
struct KgChunk {
  int i0, ic, kc, kpad, nkt, nb;  // KfChunk's fields, and the bases per input
  __device__ __forceinline__ int col(int kk, int in) const { return kk < ic ? i0 + kk : in + nb * i0 + (kk - ic); }
};
__device__ __forceinline__ KgChunk kg_chunk(int i0, int in, const KgDims& d) {
  const int ic = in - i0 < d.ic ? in - i0 : d.ic, kc = d.k1 * ic, kpad = (kc + 15) & ~15;
  return KgChunk{i0, ic, kc, kpad, kpad >> 4, d.nb};
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
      const int s = kan_bases_window<false, false, KAN_SPAN_BISECT>(x, gk + ii * d.gst, d.ng, w, unused, inv + ii * d.vst);
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
    s = kan_bases_window<DERIV, false, KAN_SPAN_BISECT>(x, h.gk + lane * d.gst, d.ng, w, dw, h.inv + lane * d.vst);
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
    const KanHeadG hg = kan_head_g<SRC>(v, yc, n < n_valid, gfac, sse);
    const float gn = hg.gn;
    sse = hg.sse;
    if (!GIVEN && lane == 0) {
      out[n] = hg.o;
      g[n] = gn;
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
    if (!GIVEN && lane == 0) sse_part[blockIdx.x] = kan_head_sse(sse_w);
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
    const int s = kan_bases_window<false, true, KAN_SPAN_BISECT>(x, gk + ii * d.gst, d.ng, w, unused, nullptr);
    As[ii][r] = silu(x);
    if (s < 0) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = s - 3 + q;
      if (c >= 0 && c < d.nb) As[ch.ic + d.nb * ii + c][r] = w[q];
    }
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
  kf_store_slab(slab, z, acc, ch.nkt, li, o0 + 16 * wv + 4 * lk, ch, in, out, d.k1);
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
      const int s = kan_bases_window<true, true, KAN_SPAN_BISECT>(x, gk + ii * d.gst, d.ng, w, dw, nullptr);
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

// W[o][i] = base_w[o][i];  W[o][in + nb i + c] = spline_w[o][i][c] * scaler[o][i]  (kan.py:145-151), and
// (WT != null) its transpose; nb bases per input (k1 = nb + 1 columns).  One body for both kernel sets:
// NB = 0 takes nb at run time, NB = KAN_NB is grid 5's instance with the loop unrolled (with the
// run-time loop at grid 5, cfg5's kan_misc measured 0.0536 against 0.0503 ms per step)
template <int NB>
__global__ void kan_combine_kernel(const float* __restrict__ base_w, const float* __restrict__ spline_w,
                                   const float* __restrict__ scaler, int out, int in, int nb_rt,
                                   float* __restrict__ W, float* __restrict__ WT) {
  const int nb = NB ? NB : nb_rt;
  const int total = out * in;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int o = e / in, i = e - o * in;
    float* row = W + (int64_t)o * (nb + 1) * in;
    row[i] = base_w[e];
    if (WT) WT[(int64_t)i * out + o] = base_w[e];
    const float s = scaler[e];
#pragma unroll NB ? NB : 1
    for (int c = 0; c < nb; ++c) {
      const float v = spline_w[(int64_t)e * nb + c] * s;
      row[in + nb * i + c] = v;
      if (WT) WT[(int64_t)(in + nb * i + c) * out + o] = v;
    }
  }
}

// Parameter gradients from dW = dLoss/dW_combined (the autograd of kan_combine):
//   d base_w = dW_base;  d spline_w = dW_spline * scaler;  d scaler = sum_c dW_spline * spline_w
template <int NB>
__global__ void kan_param_grads_kernel(const float* __restrict__ dW, const float* __restrict__ spline_w,
                                       const float* __restrict__ scaler, int out, int in, int nb_rt, int accumulate,
                                       float* __restrict__ g_base, float* __restrict__ g_spline,
                                       float* __restrict__ g_scaler) {
  const int nb = NB ? NB : nb_rt;
  const int total = out * in;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int o = e / in, i = e - o * in;
    const float* row = dW + (int64_t)o * (nb + 1) * in;
    const float s = scaler[e];
    float gs = 0.f;
#pragma unroll NB ? NB : 1
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

// ---- the KAN entry points (siren_kernels.h): k says which set runs.  The shapes are checked here,
// once for both sets; the grid-5 launchers are kan.hip's kan5_* -----------------------------------
hipError_t kan_fwd_fused(const KanSel& k, const float* X, const float* grid, const float* W, int64_t N, int in, int out,
                         float* Y, hipStream_t s) {
  if (N <= 0 || in <= 0 || out <= 0 || !kg_grid_ok(k.G)) return hipErrorInvalidValue;
  if (!k.general) return kan5_fwd_fused(X, grid, W, N, in, out, Y, s);
  hipLaunchKernelGGL(kang_fwd_fused_kernel, dim3((unsigned)((N + KF_R - 1) / KF_R), (out + KF_O - 1) / KF_O), dim3(256),
                     0, s, X, grid, W, N, in, out, k.G, Y);
  return hipGetLastError();
}

hipError_t kan_head_fwd(const KanSel& k, const float* X, const float* grid, const float* W, int64_t N, int in, float* Y,
                        hipStream_t s) {
  if (N <= 0 || in <= 0 || in > 64 || !kg_grid_ok(k.G)) return hipErrorInvalidValue;
  if (!k.general) return kan5_head_fwd(X, grid, W, N, in, Y, s);
  const size_t lds = kg_head_lds_bytes(in, k.G, false);
  static bool raised = false;
  const hipError_t e = kg_head_lds(kang_head_fwd_kernel, lds, raised);
  if (e != hipSuccess) return e;
  const int64_t blocks = (N + 3) / 4;
  hipLaunchKernelGGL(kang_head_fwd_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), lds, s, X, grid,
                     W, N, in, k.G, Y);
  return hipGetLastError();
}

template <int SRC>
static hipError_t kang_head_launch(const KanHeadPlan& p, const float* X, const float* grid, const float* W,
                                   const float* yg, int64_t N, int in, int G, int64_t n_valid, float gfac, float* out,
                                   float* g, float* sse_part, float* slab, float* Gin, hipStream_t s) {
  const size_t lds = kg_head_lds_bytes(in, G, true);
  static bool raised = false;  // one per SRC
  const hipError_t e = kg_head_lds(kang_head_train_kernel<SRC>, lds, raised);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kang_head_train_kernel<SRC>, dim3(p.blocks), dim3(256), lds, s, X, grid, W, yg, N, in, G, n_valid,
                     gfac, p.rows_per_block, out, g, sse_part, slab, Gin);
  return hipGetLastError();
}

// The head pass for g from src (KAN_HEAD_*): kan_head_plan's blocks, then the fixed-order slab sum
// into dW
static hipError_t kan_head_pass(const KanSel& k, int src, const float* X, const float* grid, const float* W,
                                const float* yg, int64_t N, int in, int64_t n_valid, float gfac, int64_t slots,
                                int64_t max_parts, float* out, float* g, float* sse_part, float* slab, float* dW,
                                float* Gin, int* nparts, hipStream_t s) {
  if (N <= 0 || in <= 0 || in > 64 || slots < 1 || max_parts < 1 || !kg_grid_ok(k.G)) return hipErrorInvalidValue;
  const KanHeadPlan p = kan_head_plan(N, slots, max_parts);
  const hipError_t e =
      !k.general ? kan5_head_pass(src, p, X, grid, W, yg, N, in, n_valid, gfac, out, g, sse_part, slab, Gin, s)
      : (src == KAN_HEAD_GIVEN ? kang_head_launch<KAN_HEAD_GIVEN>
         : src == KAN_HEAD_L1  ? kang_head_launch<KAN_HEAD_L1>
                               : kang_head_launch<KAN_HEAD_MSE>)(p, X, grid, W, yg, N, in, k.G, n_valid, gfac, out, g,
                                                                 sse_part, slab, Gin, s);
  if (e != hipSuccess) return e;
  if (nparts) *nparts = (int)p.blocks;
  return slab_reduce(slab, (int)p.blocks, (int64_t)k.k1 * in, dW, s);
}

hipError_t kan_head_train(const KanSel& k, const float* X, const float* grid, const float* W, const float* y, int64_t N,
                          int in, int64_t n_valid, float gfac, int64_t slots, int64_t max_parts, float* out, float* g,
                          float* sse_part, float* slab, float* dW, float* Gin, int* nparts, hipStream_t s,
                          int loss_mode) {
  if (!nparts || (loss_mode != 0 && loss_mode != 1)) return hipErrorInvalidValue;
  return kan_head_pass(k, loss_mode == 1 ? KAN_HEAD_L1 : KAN_HEAD_MSE, X, grid, W, y, N, in, n_valid, gfac, slots,
                       max_parts, out, g, sse_part, slab, dW, Gin, nparts, s);
}

hipError_t kan_head_bwd(const KanSel& k, const float* X, const float* grid, const float* W, const float* g, int64_t N,
                        int in, int64_t slots, int64_t max_parts, float* slab, float* dW, float* Gin, hipStream_t s) {
  return kan_head_pass(k, KAN_HEAD_GIVEN, X, grid, W, g, N, in, N, 0.f, slots, max_parts, nullptr, nullptr, nullptr,
                       slab, dW, Gin, nullptr, s);
}

// dW[o][k] = sum_n G[n][o] A[n][k]: row slices into slabs (kf_plan_dw), then the fixed-order slab sum
hipError_t kan_dw_fused(const KanSel& k, const float* X, const float* grid, const float* G, int64_t N, int in, int out,
                        int64_t max_splits, float* slab, float* dW, hipStream_t s) {
  if (N <= 0 || in <= 0 || out <= 0 || max_splits < 1 || !kg_grid_ok(k.G)) return hipErrorInvalidValue;
  const KfDwPlan p = kf_plan_dw(N, in, out, k.general ? kg_dims(k.G).ic : KF_IC, max_splits);
  if (!p.split.blocks) return hipErrorInvalidValue;
  hipError_t e;
  if (k.general) {
    hipLaunchKernelGGL(kang_dw_fused_kernel, dim3(p.split.blocks), dim3(256), 0, s, X, grid, G, N, in, out, k.G,
                       p.split.rows_per_split, p.nchunk, p.nout, p.split.z, slab);
    e = hipGetLastError();
  } else {
    e = kan5_dw_fused(p, X, grid, G, N, in, out, slab, s);
  }
  if (e != hipSuccess) return e;
  return slab_reduce(slab, p.split.z, (int64_t)out * k.k1 * in, dW, s);
}

hipError_t kan_dx_fused(const KanSel& k, const float* X, const float* grid, const float* Gout, const float* WT,
                        int64_t N, int in, int out, float* Gin, hipStream_t s) {
  if (N <= 0 || in <= 0 || out <= 0 || !kg_grid_ok(k.G)) return hipErrorInvalidValue;
  if (!k.general) return kan5_dx_fused(X, grid, Gout, WT, N, in, out, Gin, s);
  hipLaunchKernelGGL(kang_dx_fused_kernel, dim3((unsigned)((N + KF_R - 1) / KF_R)), dim3(256), 0, s, X, grid, Gout, WT,
                     N, in, out, k.G, Gin);
  return hipGetLastError();
}

// A hidden layer's backward, dW and (Gin != null) Gin.  The grid-5 set runs both in one pass when
// out <= 64; the any-grid-size set has no one-pass backward.  Profiled as the caller's launches
// are: the one-pass backward and the input-gradient pass under KAN_PROF_DX, the weight-gradient
// pass under KAN_PROF_DW.
hipError_t kan_hidden_bwd(const KanSel& k, const float* X, const float* grid, const float* G, const float* WT,
                          int64_t N, int in, int out, int64_t max_splits, float* slab, float* dW, float* Gin,
                          hipStream_t s) {
  if (N <= 0 || in <= 0 || out <= 0 || max_splits < 1 || !kg_grid_ok(k.G)) return hipErrorInvalidValue;
  const bool one_pass = out <= KF_O && Gin && !k.general;
  prof_begin(one_pass ? KAN_PROF_DX : KAN_PROF_DW, s);
  hipError_t e = one_pass ? kan5_bwd_fused(X, grid, G, WT, N, in, out, max_splits, slab, dW, Gin, s)
                          : kan_dw_fused(k, X, grid, G, N, in, out, max_splits, slab, dW, s);
  prof_end(s);
  if (e != hipSuccess || one_pass || !Gin) return e;
  prof_begin(KAN_PROF_DX, s);
  e = kan_dx_fused(k, X, grid, G, WT, N, in, out, Gin, s);
  prof_end(s);
  return e;
}

hipError_t kan_combine(const KanSel& k, const float* base_w, const float* spline_w, const float* scaler, int out, int in,
                       float* W, float* WT, hipStream_t s) {
  if (!kg_grid_ok(k.G)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k.general ? kan_combine_kernel<0> : kan_combine_kernel<KAN_NB>, dim3(ew_grid((int64_t)out * in)),
                     dim3(256), 0, s, base_w, spline_w, scaler, out, in, k.k1 - 1, W, WT);
  return hipGetLastError();
}

hipError_t kan_param_grads(const KanSel& k, const float* dW, const float* spline_w, const float* scaler, int out, int in,
                           int accumulate, float* g_base, float* g_spline, float* g_scaler, hipStream_t s) {
  if (!kg_grid_ok(k.G)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k.general ? kan_param_grads_kernel<0> : kan_param_grads_kernel<KAN_NB>,
                     dim3(ew_grid((int64_t)out * in)), dim3(256), 0, s, dW, spline_w, scaler, out, in, k.k1 - 1,
                     accumulate, g_base, g_spline, g_scaler);
  return hipGetLastError();
}

// ---- the refit (KANLinear.update_grid, kan.py:168-215, and KANLinear.regrid) ----------------------
// The reference refits every curve on the new knots by least squares over the batch:
// min || A_new c - B ||, B[r][o] = sum_c A_old[r][c] coeff_old[o][i][c].  A_new^T B =
// (A_new^T A_old) coeff_old, so per input i, with the old and the new basis each at its own size,
//   c_new[i] = G_nn[i]^-1 G_no[i] c_old[i],  G_nn (Gn+3) x (Gn+3),  G_no (Gn+3) x (Go+3)
//   G_nn[i] = sum_r b_new(x_ri) b_new(x_ri)^T,  G_no[i] = sum_r b_new(x_ri) b_old(x_ri)^T
// and nothing of size rows x out (the reference's (batch, in, out) intermediate is 115 GB at
// 441 000 x 256 x 256).  The bases are the forward's fp32 values on IEEE quotients; their products
// are exact in fp64 and are summed in fp64 in a fixed order (no floating-point atomics), so two runs
// agree bit for bit.  update_grid is Go = Gn = grid_size with the scaler passed in.  A row touches
// 10 entries of G_nn's upper band and one 4 x 4
// block of G_no, the block of its new span s and old span r.  G_no is a staircase: two pairs of
// overlapping half-open spans never share s + r.  (Take (s, r) and (s', r') with s < s' and r > r':
// an x in the first pair and a y in the second give y >= gn[s'] >= gn[s+1] > x >= go[r] >= go[r'+1]
// > y.)  So slot t = s + r addresses a compact accumulator without collisions, of
//   E = 4 (Gn+3) + 16 (Gn + Go + 11) doubles per input: G_nn's band [c][d - c], then [t][p][k]
// (2492 at 64 -> 64, where the dense pair of matrices has 8978), and the per-slice partials have
// that size too.  At 5 -> 5 (update_grid's case) the dense pair is the smaller one, 128 doubles
// against 368, and 64 inputs fit a block where the compact accumulator lets 49 in: that pair alone
// runs kan_regrid_gram_dense5_kernel (kr_gram_plan).
//   kan_regrid_knots  the new knots from Gn + 1 order statistics of each input
//   kan_regrid_gram   row slices into fp64 partials, then a fixed-order sum into dense Grams
//   kan_regrid_refit  banded Cholesky of G_nn, M = G_nn^-1 G_no, spline_w_new = fp32(M c_old)
constexpr int KR_ROWS = 8;                                             // rows a lane loads before it evaluates them
constexpr int KR_MAX_SLICES = 256, KR_MIN_SLICES = 8, KR_BLOCKS = 1024;
constexpr size_t kKrLdsMax = 160 * 1024;
constexpr int KR_DENSE5_E = 2 * KAN_NB * KAN_NB;  // the 5 -> 5 Gram's fp64 entries per input: G_nn then G_no, [8][8] each

struct KrDims {
  KgDims o, n;  // the old and the new grid
  int nn, e;    // doubles of G_nn's band; of one input's compact accumulator
};
__host__ __device__ constexpr KrDims kr_dims(int Go, int Gn) {
  return KrDims{kg_dims(Go), kg_dims(Gn), 4 * (Gn + 3), 4 * (Gn + 3) + 16 * (Gn + Go + 11)};
}
// LDS of one input: its accumulator, both knot rows and both reciprocal tables
__host__ __device__ constexpr size_t kr_lds_per_input(const KrDims& d) {
  return sizeof(double) * d.e + sizeof(float) * (d.o.gst + d.n.gst + d.o.vst + d.n.vst);
}
// inputs of a block (one wave, lane = input): what fits the CU's LDS, 64 at the most
__host__ __device__ constexpr int kr_ic(const KrDims& d) {
  return (int)(kKrLdsMax / kr_lds_per_input(d) < 64 ? kKrLdsMax / kr_lds_per_input(d) : 64);
}
static_assert(kr_ic(kr_dims(KG_MAX_GRID, KG_MAX_GRID)) >= 1, "one input's accumulator outgrows the LDS");

// kan.py:183-212 op for op in fp32 (IEEE division; each product rounded before the sum), Gn for its 5:
//   step = (x_last - x_first + 2 margin) / Gn
//   knot_k = eps ((k step + x_first) - margin) + (1 - eps) q_k,  k = 0..Gn
// extended by three steps on either side.  q[k][i]: the k-th of the Gn + 1 order statistics of input i.
__global__ __launch_bounds__(256) void kan_regrid_knots_kernel(const float* __restrict__ q, int in, int Gn, float margin,
                                                               float margin2, float eps, float one_eps,
                                                               float* __restrict__ grid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= in) return;
  const float x0 = q[i], xl = q[Gn * (int64_t)in + i];
  const float step = ((xl - x0) + margin2) / (float)Gn;
  float* out = grid + (int64_t)i * (Gn + 7);
  float g0 = 0.f, gl = 0.f;
  for (int k = 0; k <= Gn; ++k) {
    const float gu = ((float)k * step + x0) - margin;
    const float g = eps * gu + one_eps * q[k * (int64_t)in + i];
    out[3 + k] = g;
    g0 = k == 0 ? g : g0;
    gl = g;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = g0 - step * (float)(3 - k);
#pragma unroll
  for (int k = 1; k <= 3; ++k) out[Gn + 3 + k] = gl + step * (float)k;
}

// The compact Gram at run-time sizes: one wave per block, lane = input i0 + lane of the
// block's ic = kr_ic inputs (X rows are read along the lanes, each element once).  Dynamic LDS:
//   acc [E][ic] doubles (lane-consecutive: no bank conflicts whatever the spans), then
//   gk_o [ic][gst_o]  gk_n [ic][gst_n]  inv_o [ic][vst_o]  inv_n [ic][vst_n] floats.
// Block (cg, z) takes the 8-row tiles z, z + Z, ... and writes part[z][e][i] for every e.
__global__ __launch_bounds__(64) void kan_regrid_gram_kernel(const float* __restrict__ X,
                                                             const float* __restrict__ grid_old,
                                                             const float* __restrict__ grid_new, int64_t N, int in,
                                                             int Go, int Gn, int icb, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double kr_smem[];
  const KrDims d = kr_dims(Go, Gn);
  const int lane = threadIdx.x, i0 = blockIdx.x * icb;
  const int ic = in - i0 < icb ? in - i0 : icb;
  double* acc = kr_smem;
  float* gko = reinterpret_cast<float*>(acc + (size_t)d.e * icb);
  float* gkn = gko + icb * d.o.gst;
  float* ivo = gkn + icb * d.n.gst;
  float* ivn = ivo + icb * d.o.vst;
  kg_fill_knots(gko, grid_old, i0, ic, d.o);
  kg_fill_knots(gkn, grid_new, i0, ic, d.n);
  kg_fill_inv(ivo, grid_old, i0, ic, d.o);
  kg_fill_inv(ivn, grid_new, i0, ic, d.n);
  for (int e = lane; e < d.e * icb; e += 64) acc[e] = 0.0;
  __syncthreads();
  const bool on = lane < ic;
  double* a = acc + lane;  // a[e * icb]
  const int nbn = d.n.nb, nbo = d.o.nb;
  const int64_t ntile = (N + KR_ROWS - 1) / KR_ROWS;
  for (int64_t t = blockIdx.y; t < ntile; t += gridDim.y) {
    float x[KR_ROWS];
#pragma unroll
    for (int r = 0; r < KR_ROWS; ++r) {
      const int64_t n = t * KR_ROWS + r;
      x[r] = (on && n < N) ? X[n * in + i0 + lane] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < KR_ROWS; ++r) {
      if (!on || t * KR_ROWS + r >= N) continue;
      float wn[4], wo[4], unused[4];
      const int sn = kan_bases_window<false, false, KAN_SPAN_BISECT>(x[r], gkn + lane * d.n.gst, d.n.ng, wn, unused, ivn + lane * d.n.vst);
      if (sn < 0) continue;
      const int so = kan_bases_window<false, false, KAN_SPAN_BISECT>(x[r], gko + lane * d.o.gst, d.o.ng, wo, unused, ivo + lane * d.o.vst);
      double* blk = a + (int64_t)(d.nn + 16 * (sn + (so < 0 ? 0 : so))) * icb;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int c = sn - 3 + p;
        if (c < 0 || c >= nbn) continue;
        const double bp = (double)wn[p];
#pragma unroll
        for (int k = p; k < 4; ++k)
          if (sn - 3 + k < nbn) a[(4 * c + (k - p)) * icb] += bp * (double)wn[k];
        if (so >= 0) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int dd = so - 3 + k;
            if (dd >= 0 && dd < nbo) blk[(4 * p + k) * icb] += bp * (double)wo[k];
          }
        }
      }
    }
  }
  if (!on) return;
  double* out = part + (int64_t)blockIdx.y * d.e * in + i0 + lane;
  for (int e = 0; e < d.e; ++e) out[(int64_t)e * in] = a[e * icb];
}

// gram[i] = {G_nn [NBn][NBn], G_no [NBn][NBo]} = (accumulate ? gram[i] : 0) + the slices in order.
// One thread per dense entry.  G_nn (c, d): the band entry (min, |c - d|), an exact zero outside the
// band.  G_no (c, d): the blocks of the spans s = c + 3 - p, r = d + 3 - k that overlap on this
// input's knots (the only ones a row can have hit; each has its own slot s + r), in (p, k) order.
__global__ __launch_bounds__(256) void kan_regrid_gram_reduce_kernel(const double* __restrict__ part, int slices, int in,
                                                                     int Go, int Gn, const float* __restrict__ grid_old,
                                                                     const float* __restrict__ grid_new, int accumulate,
                                                                     double* __restrict__ gram) {
  const KrDims d = kr_dims(Go, Gn);
  const int nbn = d.n.nb, nbo = d.o.nb, per = nbn * (nbn + nbo);
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)per * in) return;
  const int e = (int)(idx / in), i = (int)(idx - (int64_t)e * in);
  double* dst = gram + (int64_t)i * per + e;
  double v = accumulate ? *dst : 0.0;
  const int64_t zs = (int64_t)d.e * in;
  if (e < nbn * nbn) {
    const int c = e / nbn, dd = e - c * nbn, lo = c < dd ? c : dd, w = c < dd ? dd - c : c - dd;
    if (w <= 3) {
      const double* p = part + (int64_t)(4 * lo + w) * in + i;
      for (int z = 0; z < slices; ++z) v += p[z * zs];
    }
  } else {
    const int f = e - nbn * nbn, c = f / nbo, dd = f - c * nbo;
    const float* go = grid_old + (int64_t)i * d.o.ng;
    const float* gn = grid_new + (int64_t)i * d.n.ng;
    for (int p = 0; p < 4; ++p) {
      const int s = c + 3 - p;
      if (s > d.n.ng - 2) continue;
      for (int k = 0; k < 4; ++k) {
        const int r = dd + 3 - k;
        if (r > d.o.ng - 2) continue;
        const float lo = gn[s] > go[r] ? gn[s] : go[r], hi = gn[s + 1] < go[r + 1] ? gn[s + 1] : go[r + 1];
        if (!(lo < hi)) continue;
        const double* q = part + (int64_t)(d.nn + 16 * (s + r) + 4 * p + k) * in + i;
        for (int z = 0; z < slices; ++z) v += q[z * zs];
      }
    }
  }
  *dst = v;
}

// The dense case, Go = Gn = 5 (kan.hip's compile-time tables).  One wave per block; lane = input
// i0 + lane (X rows are read along the lanes: coalesced, each element once).
// The lane's 128 fp64 sums live in LDS as acc[e][lane] (the entries a row touches
// depend on its spans, so registers will not do; lane-consecutive doubles: no bank conflicts
// whatever the spans).  Block (cg, z) takes the 8-row tiles z, z + Z, ... of its 64 inputs and
// writes part[z][e][i]; G_nn is summed on its upper triangle and mirrored on the way out, and the
// entries no row touches (|c - d| > 3) stay exact zeros.
__global__ __launch_bounds__(64) void kan_regrid_gram_dense5_kernel(const float* __restrict__ X,
                                                                    const float* __restrict__ grid_old,
                                                                    const float* __restrict__ grid_new, int64_t N,
                                                                    int in, double* __restrict__ part) {
  __shared__ double acc[KR_DENSE5_E][64];
  __shared__ float gk[2][64][KF_GST];
  __shared__ float inv[2][64][KF_VST];
  const int lane = threadIdx.x, i0 = blockIdx.x * 64;
  const int ic = in - i0 < 64 ? in - i0 : 64;
  kf_fill_knots(gk[0], grid_old, i0, ic);
  kf_fill_knots(gk[1], grid_new, i0, ic);
  kf_fill_inv(inv[0], grid_old, i0, ic);
  kf_fill_inv(inv[1], grid_new, i0, ic);
#pragma unroll 8
  for (int e = 0; e < KR_DENSE5_E; ++e) acc[e][lane] = 0.0;
  __syncthreads();
  const bool on = lane < ic;
  const int64_t ntile = (N + KR_ROWS - 1) / KR_ROWS;
  for (int64_t t = blockIdx.y; t < ntile; t += gridDim.y) {
    float x[KR_ROWS];
#pragma unroll
    for (int r = 0; r < KR_ROWS; ++r) {
      const int64_t n = t * KR_ROWS + r;
      x[r] = (on && n < N) ? X[n * in + i0 + lane] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < KR_ROWS; ++r) {
      if (!on || t * KR_ROWS + r >= N) continue;
      float wn[4], wo[4], unused[4];
      const int sn = kan_bases_window<false, false, KAN_SPAN_SELECT>(x[r], gk[1][lane], KAN_NG, wn, unused, inv[1][lane]);
      if (sn < 0) continue;
      const int so = kan_bases_window<false, false, KAN_SPAN_SELECT>(x[r], gk[0][lane], KAN_NG, wo, unused, inv[0][lane]);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int c = sn - 3 + p;
        if (c < 0 || c >= KAN_NB) continue;
        const double bp = (double)wn[p];
#pragma unroll
        for (int k = p; k < 4; ++k) {
          const int d = sn - 3 + k;
          if (d < KAN_NB) acc[c * KAN_NB + d][lane] += bp * (double)wn[k];
        }
        if (so >= 0) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int d = so - 3 + k;
            if (d >= 0 && d < KAN_NB) acc[KAN_NB * KAN_NB + c * KAN_NB + d][lane] += bp * (double)wo[k];
          }
        }
      }
    }
  }
  if (!on) return;
  double* out = part + (int64_t)blockIdx.y * KR_DENSE5_E * in + i0 + lane;
  for (int c = 0; c < KAN_NB; ++c)
    for (int d = 0; d < KAN_NB; ++d) {
      out[(int64_t)(c * KAN_NB + d) * in] = c <= d ? acc[c * KAN_NB + d][lane] : acc[d * KAN_NB + c][lane];
      out[(int64_t)(KAN_NB * KAN_NB + c * KAN_NB + d) * in] = acc[KAN_NB * KAN_NB + c * KAN_NB + d][lane];
    }
}

// gram[i][e] = (accumulate ? gram[i][e] : 0) + part[0][e][i] + part[1][e][i] + ... in slice order
__global__ __launch_bounds__(256) void kan_regrid_gram_dense5_reduce_kernel(const double* __restrict__ part, int slices,
                                                                            int in, int accumulate,
                                                                            double* __restrict__ gram) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)KR_DENSE5_E * in) return;
  const int e = (int)(idx / in), i = (int)(idx - (int64_t)e * in);
  double v = accumulate ? gram[(int64_t)i * KR_DENSE5_E + e] : 0.0;
  for (int z = 0; z < slices; ++z) v += part[(int64_t)z * KR_DENSE5_E * in + idx];
  gram[(int64_t)i * KR_DENSE5_E + e] = v;
}

// One block per input.  Dynamic LDS: Lb [NBn + 3][4] doubles, the banded Cholesky factor
// Lb[r][r - j] = L[r][j] (j = r-3 .. r; entries off the matrix and three rows past it are zeros, so
// the substitutions need no edge cases), Ab [NBn][4], G_nn's lower band in the same layout, then
// M [NBn][NBo], G_no solved in place.
//   thread 0      G_nn = L L^T in fp64, in the dense factorisation's order less its exact-zero terms
//   thread c      column c of G_no: L y = b, L^T x = y, three values of y (x) back in registers
//   thread o, ..  spline_w_new[o][i][:] = fp32(M (spline_w[o][i][:] * scaler[o][i])); with a scaler
//                 (update_grid) the refit targets the scaled curves and the result is stored
//                 undivided (kan.py:175, :215)
// A pivot at or below 2^-40 x the largest diagonal entry (or a NaN) marks the input rank deficient:
// it counts in status[0], lowers status[1] to its index and writes nothing.
__global__ __launch_bounds__(256) void kan_regrid_refit_kernel(const double* __restrict__ gram, int in, int out, int Go,
                                                               int Gn, const float* __restrict__ spline_w,
                                                               const float* __restrict__ scaler,
                                                               float* __restrict__ spline_w_new,
                                                               int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double kr_smem[];
  __shared__ int ok_s;
  const int nbn = Gn + 3, nbo = Go + 3, i = blockIdx.x, tid = threadIdx.x;
  const double* Gnn = gram + (int64_t)i * nbn * (nbn + nbo);
  const double* Gno = Gnn + nbn * nbn;
  double* Lb = kr_smem;
  double* Ab = Lb + 4 * (nbn + 3);  // Ab[r][r - j] = G_nn[r][j], its lower band
  double* M = Ab + 4 * nbn;
  for (int e = tid; e < 4 * (nbn + 3); e += blockDim.x) Lb[e] = 0.0;
  for (int e = tid; e < 4 * nbn; e += blockDim.x) {
    const int r = e >> 2, j = r - (e & 3);
    Ab[e] = j >= 0 ? Gnn[r * nbn + j] : 0.0;
  }
  for (int e = tid; e < nbn * nbo; e += blockDim.x) M[e] = Gno[e];
  __syncthreads();
  if (tid == 0) {
    double dmax = 0.0;
    for (int c = 0; c < nbn; ++c) dmax = Ab[4 * c] > dmax ? Ab[4 * c] : dmax;
    const double thr = dmax * 0x1p-40;
    bool ok = dmax > 0.0;
    for (int j = 0; j < nbn && ok; ++j) {
      double p = Ab[4 * j];
      for (int k = j < 3 ? 0 : j - 3; k < j; ++k) p -= Lb[4 * j + (j - k)] * Lb[4 * j + (j - k)];
      if (!(p > thr)) {
        ok = false;
        break;
      }
      const double l = sqrt(p);
      Lb[4 * j] = l;
      for (int r = j + 1; r < nbn && r <= j + 3; ++r) {
        double v = Ab[4 * r + (r - j)];
        for (int k = r < 3 ? 0 : r - 3; k < j; ++k) v -= Lb[4 * r + (r - k)] * Lb[4 * j + (j - k)];
        Lb[4 * r + (r - j)] = v / l;
      }
    }
    if (!ok) {
      atomicAdd(&status[0], 1);
      atomicMin(&status[1], i);
    }
    ok_s = ok ? 1 : 0;
  }
  __syncthreads();
  if (!ok_s) return;  // the whole block
  for (int c = tid; c < nbo; c += blockDim.x) {
    double y1 = 0.0, y2 = 0.0, y3 = 0.0;  // y[r-1], y[r-2], y[r-3]
    for (int r = 0; r < nbn; ++r) {
      const double* l = Lb + 4 * r;
      double v = M[r * nbo + c];
      v -= l[3] * y3;
      v -= l[2] * y2;
      v -= l[1] * y1;
      v /= l[0];
      M[r * nbo + c] = v;
      y3 = y2, y2 = y1, y1 = v;
    }
    double x1 = 0.0, x2 = 0.0, x3 = 0.0;  // x[r+1], x[r+2], x[r+3]
    for (int r = nbn - 1; r >= 0; --r) {
      double v = M[r * nbo + c];
      v -= Lb[4 * (r + 1) + 1] * x1;
      v -= Lb[4 * (r + 2) + 2] * x2;
      v -= Lb[4 * (r + 3) + 3] * x3;
      v /= Lb[4 * r];
      M[r * nbo + c] = v;
      x3 = x2, x2 = x1, x1 = v;
    }
  }
  __syncthreads();
  for (int o = tid; o < out; o += blockDim.x) {
    const int64_t idx = (int64_t)o * in + i;
    const float s = scaler ? scaler[idx] : 1.0f;
    const float* w = spline_w + idx * nbo;
    float* wn = spline_w_new + idx * nbn;
    for (int r = 0; r < nbn; ++r) {
      const double* m = M + r * nbo;
      double a = 0.0;
      for (int c = 0; c < nbo; ++c) a += m[c] * (double)(w[c] * s);
      wn[r] = (float)a;
    }
  }
}

static bool kr_grids_ok(int Go, int Gn) { return kg_grid_ok(Go) && kg_grid_ok(Gn); }

hipError_t kan_regrid_knots(const float* q, int in, int Gn, float margin, float margin2, float eps, float one_eps,
                            float* grid, hipStream_t s) {
  if (in <= 0 || !kg_grid_ok(Gn)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kan_regrid_knots_kernel, dim3((in + 255) / 256), dim3(256), 0, s, q, in, Gn, margin, margin2, eps,
                     one_eps, grid);
  return hipGetLastError();
}

// Which Gram kernel a pair of sizes runs, and what follows from it: the inputs of a block and the
// doubles per slice and input.  Compact: kr_ic inputs, and no more than the layer has (a narrow
// layer asks for less LDS).
struct KrGramPlan {
  bool dense5;
  int icb, e;
};
static KrGramPlan kr_gram_plan(int in, int Go, int Gn) {
  if (Go == 5 && Gn == 5) return KrGramPlan{true, 64, KR_DENSE5_E};
  const KrDims d = kr_dims(Go, Gn);
  return KrGramPlan{false, in < kr_ic(d) ? in : kr_ic(d), d.e};
}

// row slices of the Gram kernel: about KR_BLOCKS one-wave blocks over the column groups
int kan_regrid_slices(int64_t N, int in, int Go, int Gn) {
  const int icb = kr_gram_plan(in, Go, Gn).icb, ncg = (in + icb - 1) / icb;
  int z = KR_BLOCKS / ncg;
  z = z < KR_MIN_SLICES ? KR_MIN_SLICES : (z > KR_MAX_SLICES ? KR_MAX_SLICES : z);
  const int64_t ntile = (N + KR_ROWS - 1) / KR_ROWS;
  return ntile < z ? (int)(ntile < 1 ? 1 : ntile) : z;
}
int64_t kan_regrid_pass_rows(int in, int Go, int Gn) {
  return (int64_t)KR_ROWS * kan_regrid_slices(INT64_MAX / 2, in, Go, Gn);
}
int64_t kan_regrid_part_doubles(int64_t N, int in, int Go, int Gn) {
  return (int64_t)kan_regrid_slices(N, in, Go, Gn) * kr_gram_plan(in, Go, Gn).e * in;
}

hipError_t kan_regrid_gram(const float* X, const float* grid_old, const float* grid_new, int64_t N, int in, int Go,
                           int Gn, int accumulate, double* part, double* gram, hipStream_t s) {
  if (N <= 0 || in <= 0 || !kr_grids_ok(Go, Gn)) return hipErrorInvalidValue;
  const KrGramPlan plan = kr_gram_plan(in, Go, Gn);
  const int icb = plan.icb, z = kan_regrid_slices(N, in, Go, Gn);
  if (plan.dense5) {
    hipLaunchKernelGGL(kan_regrid_gram_dense5_kernel, dim3((in + 63) / 64, z), dim3(64), 0, s, X, grid_old, grid_new, N,
                       in, part);
    hipLaunchKernelGGL(kan_regrid_gram_dense5_reduce_kernel, dim3((unsigned)(((int64_t)KR_DENSE5_E * in + 255) / 256)),
                       dim3(256), 0, s, part, z, in, accumulate, gram);
    return hipGetLastError();
  }
  const KrDims d = kr_dims(Go, Gn);
  const size_t lds = kr_lds_per_input(d) * icb;
  static bool raised = false;
  const hipError_t e = kg_head_lds(kan_regrid_gram_kernel, lds, raised);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kan_regrid_gram_kernel, dim3((in + icb - 1) / icb, z), dim3(64), lds, s, X, grid_old, grid_new, N,
                     in, Go, Gn, icb, part);
  const int64_t total = (int64_t)d.n.nb * (d.n.nb + d.o.nb) * in;
  hipLaunchKernelGGL(kan_regrid_gram_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, z, in,
                     Go, Gn, grid_old, grid_new, accumulate, gram);
  return hipGetLastError();
}

hipError_t kan_regrid_refit(const double* gram, int in, int out, int Go, int Gn, const float* spline_w,
                            const float* scaler, float* spline_w_new, int* status, hipStream_t s) {
  if (in <= 0 || out <= 0 || !kr_grids_ok(Go, Gn)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int), s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(status + 1, 0x7f, sizeof(int), s);  // above every index
  if (e != hipSuccess) return e;
  const size_t lds = sizeof(double) * (4 * (Gn + 6) + 4 * (Gn + 3) + (size_t)(Gn + 3) * (Go + 3));  // 40 KB at 64 -> 64
  hipLaunchKernelGGL(kan_regrid_refit_kernel, dim3(in), dim3(256), lds, s, gram, in, out, Go, Gn, spline_w, scaler,
                     spline_w_new, status);
  return hipGetLastError();
}

}  // namespace siren
