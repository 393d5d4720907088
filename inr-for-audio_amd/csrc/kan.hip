// KAN path: efficient-KAN `KANLinear` layers (kan.py:6-166):
//   A = [ SiLU(X) | B-spline bases of X ]   [N][9 in]   (grid 5, order 3)
//   Out = A W^T,  W = [ base_weight | spline_weight * spline_scaler ]  [out][9 in]
// and its autograd: dW = G^T A, dA = G W, dX = SiLU'(X) dA_base + sum_c B'_c(X) dA_spline_c.
//
// A and dA are never materialised (round 2; the first design wrote and re-read A / dA, 2.3 KB
// per coordinate each at width 64, ~26 KB of HBM per coordinate-step).  The fused kernels
// recompute the bases of a (16-input x 64-row) chunk (KfChunk) into LDS where they are consumed:
//   kan_fwd_fused  Out tile [64 rows][64 outs] = sum over input chunks of A_chunk W_chunk^T
//   kan_dw_fused   dW chunk [out][144] += G[rows]^T A_chunk[rows]   (split-K over rows, slabs)
//   kan_dx_fused   dA_chunk = G W_chunk (in LDS), contracted at once with the bases' derivatives
//   kan_bwd_fused  both backward products of a chunk in one pass (out <= 64)
//   kan_head_fwd / kan_head_train / kan_head_bwd  the last layer (out = 1): inference; forward,
//                  MSE or L1 gradient and backward in one pass; the backward alone for a given
//                  g (one row evaluation for all: kan_head_row)
// These kernels are grid_size 5's (KAN_NB = 8 at compile time).  Every other grid size runs their twins in
// kan_general.hip, which also holds the entry points of both sets (they reach this file through the
// kan5_* launchers at its end), kan_combine / kan_param_grads, and the refit of update_grid and regrid
// (kan_regrid_*) for every size, 5 included.  Both files take their tool kit from kan_tiles.h.
// The three backward kernels are put together from one set of tile helpers: kf_fill_a (A tile;
// kan_bwd_fused keeps its own, with the derivatives in registers),
// kf_g_load / kf_g_store / kf_g_scalar (G tile), kf_load_wt (W^T chunk), kf_da_to_gin (dA -> Gin),
// kf_split_block / kf_store_slab / kf_plan_splits (row splits and their slabs).
// Everything is fp32 like the reference.  The bases follow kan.py:94-104's Cox-de Boor
// recursion op for op (sub, div, mul, add; fp-contract off) on the layer's own `grid` buffer,
// so they are bit-identical to torch's CPU result; the derivative differentiates the same
// recursion.  The chunk products run on the f32-input MFMA (exact f32); the last
// layer (out = 1) is a per-row dot product on the VALU (kan_head_*).
#include "kan_tiles.h"

namespace siren {

// As[r][ii] = SiLU(x), As[r][ic + 8 ii + c] = B_c(x) for the pair (r, ii) (zeros for rows past N)
__device__ __forceinline__ void kf_put_pair(float (*As)[KF_AST], int r, int ii, int ic, float x, bool valid,
                                            const float (*gk)[KF_GST], const float (*inv)[KF_VST]) {
  float b[KAN_NB], unused[KAN_NB], sl = 0.f;
  if (valid) {
    kan_bases_local<false>(x, gk[ii], b, unused, inv[ii]);
    sl = silu(x);
  } else {
#pragma unroll
    for (int c = 0; c < KAN_NB; ++c) b[c] = 0.f;
  }
  As[r][ii] = sl;
  float* d = &As[r][ic + 8 * ii];
  if ((ic & 3) == 0) {
    *reinterpret_cast<float4*>(d) = float4{b[0], b[1], b[2], b[3]};
    *reinterpret_cast<float4*>(d + 4) = float4{b[4], b[5], b[6], b[7]};
  } else {
#pragma unroll
    for (int c = 0; c < KAN_NB; ++c) d[c] = b[c];
  }
}

// Y[n][o] = sum_k A[n][k] W[o][k]; grid (ceil(N/64), ceil(out/64)).  Wave w: rows 16w .. 16w+15
// x 64 outs (4 accumulators), K = the chunk's kpad columns, summed over the chunks.
__global__ __launch_bounds__(256) void kan_fwd_fused_kernel(const float* __restrict__ X, const float* __restrict__ grid,
                                                            const float* __restrict__ W, int64_t N, int in, int out,
                                                            float* __restrict__ Y) {
  __shared__ __attribute__((aligned(16))) float As[KF_R][KF_AST];  // [row][kk]
  __shared__ __attribute__((aligned(16))) float Ws[KF_O][KF_AST];  // [o][kk]
  __shared__ float gk[KF_IC][KF_GST];
  __shared__ float inv[KF_IC][KF_VST];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * KF_R;
  const int o0 = blockIdx.y * KF_O;
  const int64_t K = (int64_t)KAN_K1 * in;
  const bool vec = (in & 3) == 0 && in % KF_IC == 0;  // every chunk full, 16-byte pieces
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // vec path: a chunk's W pieces (4 SiLU + 32 spline 16-byte pieces per out) and X piece, loaded
  // into registers one chunk ahead so their latency hides under the previous chunk's products
  const int xr = tid >> 2, xi = (tid & 3) * 4;
  float4 wv4[9], xv4 = float4{0.f, 0.f, 0.f, 0.f};
  auto load_chunk = [&](int i0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      const int idx = tid + 256 * q, o = idx / 36, c4 = idx % 36;
      const int64_t col = c4 < 4 ? i0 + 4 * c4 : in + 8 * i0 + 4 * (c4 - 4);
      wv4[q] = o0 + o < out ? ldg4(W + (int64_t)(o0 + o) * K + col) : float4{0.f, 0.f, 0.f, 0.f};
    }
    xv4 = r0 + xr < N ? ldg4(X + (r0 + xr) * in + i0 + xi) : float4{0.f, 0.f, 0.f, 0.f};
  };
  if (vec) load_chunk(0);
  for (int i0 = 0; i0 < in; i0 += KF_IC) {
    const KfChunk ch = kf_chunk(i0, in);
    const int ic = ch.ic, kc = ch.kc, kpad = ch.kpad;
    kf_fill_knots(gk, grid, i0, ic);
    kf_fill_inv(inv, grid, i0, ic);
    // W chunk as Ws[o][kk]: from W's rows, unlike the backward's kf_load_wt
    if (vec) {
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const int idx = tid + 256 * q, o = idx / 36, c4 = idx % 36;
        *reinterpret_cast<float4*>(&Ws[o][4 * c4]) = wv4[q];
      }
    } else {
      for (int e = tid; e < KF_O * kpad; e += blockDim.x) {
        const int o = e / kpad, kk = e - o * kpad;
        Ws[o][kk] = (o0 + o < out && kk < kc) ? W[(int64_t)(o0 + o) * K + ch.col(kk, in)] : 0.f;
      }
      for (int e = tid; e < (kpad - kc) * KF_R; e += blockDim.x) As[e % KF_R][kc + e / KF_R] = 0.f;
    }
    __syncthreads();
    // A tile: the vec path's thread computes the 4 pairs whose x it loaded
    if (vec) {
      const bool valid = r0 + xr < N;
      kf_put_pair(As, xr, xi, ic, xv4.x, valid, gk, inv);
      kf_put_pair(As, xr, xi + 1, ic, xv4.y, valid, gk, inv);
      kf_put_pair(As, xr, xi + 2, ic, xv4.z, valid, gk, inv);
      kf_put_pair(As, xr, xi + 3, ic, xv4.w, valid, gk, inv);
    } else {
      for (int p = tid; p < KF_R * ic; p += blockDim.x) {
        const int r = p & (KF_R - 1), ii = p >> 6;
        const bool valid = r0 + r < N;
        kf_put_pair(As, r, ii, ic, valid ? X[(r0 + r) * in + i0 + ii] : 0.f, valid, gk, inv);
      }
    }
    __syncthreads();
    if (vec && i0 + KF_IC < in) load_chunk(i0 + KF_IC);
    if ((KAN_ABL & 2) == 0)
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

// ---- the last layer (out = 1, in <= 64): one wave per row, lane = input ----------------------
// out[n] = SiLU(x_lane) W[lane] + sum_c B_c(x_lane) W[in + 8 lane + c], summed over the wave in a
// fixed butterfly order.  kan_head_fwd and kan_head_train share the set-up and the row evaluation,
// so the training pass's out is the inference's bit for bit.
struct KanHeadLane {  // lane i's weights: W[i] and W[in + 8 i + c] (zero for the lanes past in)
  float wb, ws[KAN_NB];
};

// the block's knots and reciprocals into LDS, and the lane's weights
__device__ __forceinline__ KanHeadLane kan_head_setup(float (*gk)[KF_GST], float (*inv)[KF_VST],
                                                      const float* __restrict__ grid, const float* __restrict__ W,
                                                      int in) {
  kf_fill_knots(gk, grid, 0, in);
  kf_fill_inv(inv, grid, 0, in);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  KanHeadLane w = {};
  if (lane < in) {
    w.wb = W[lane];
#pragma unroll
    for (int c = 0; c < KAN_NB; ++c) w.ws[c] = W[in + KAN_NB * lane + c];
  }
  return w;
}

// the row's output on every lane, from lane i's input x (read when `on`: i < in); on those lanes
// also sl = SiLU(x), b[] = B(x) and, with DERIV, dsl = SiLU'(x) and db[] = B'(x)
template <bool DERIV>
__device__ __forceinline__ float kan_head_row(bool on, float x, const float* g, const float* inv, const KanHeadLane& w,
                                              float& sl, float& dsl, float* b, float* db) {
  float v = 0.f;
  if (on) {
    kan_bases_local<DERIV, false, KAN_SPAN_SELECT>(x, g, b, db, inv);  // lane-fixed knots: selects
    if constexpr (DERIV) silu_and_grad(x, sl, dsl);
    else sl = silu(x);
    v = sl * w.wb;
#pragma unroll
    for (int c = 0; c < KAN_NB; ++c) v += b[c] * w.ws[c];
  }
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void kan_head_fwd_kernel(const float* __restrict__ X, const float* __restrict__ grid,
                                                           const float* __restrict__ W, int64_t N, int in,
                                                           float* __restrict__ Y) {
  __shared__ float gk[64][KF_GST];
  __shared__ float inv[64][KF_VST];
  const KanHeadLane w = kan_head_setup(gk, inv, grid, W, in);
  const int lane = threadIdx.x & 63;
  const bool on = lane < in;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t n = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); n < N; n += nw) {
    float sl, unused, b[KAN_NB], db[KAN_NB];
    const float v = kan_head_row<false>(on, on ? X[n * in + lane] : 0.f, gk[lane], inv[lane], w, sl, unused, b, db);
    if (lane == 0) Y[n] = v;
  }
}

// Training pass of the last layer (out = 1, in <= 64) over its rows.  Per row: the
// forward out = SiLU(x) W[i] + sum_c B_c(x) W[in + 8 i + c] through kan_head_row like
// kan_head_fwd (so out is bit-identical to inference), the loss gradient g and the loss partial
// (rows >= n_valid contribute nothing), then the backward: Gin[n][i]
// = g_n (SiLU'(x) W[i] + sum_c B'_c(x) W[in + 8 i + c]) (dA = g W is a rank-1 product, never
// formed) and the weight-gradient partials -- one basis evaluation per (row, input) for the
// forward and the backward, and no pass over X or out between them.  Blocks take >= 256 contiguous rows (one
// slab row and one loss partial each); their 4 waves take every 4th row.
// SRC says where g comes from:
//   KAN_HEAD_MSE    g = 2 (out - y) / N, partial err^2              (run.py:160, :168 nn.MSELoss)
//   KAN_HEAD_L1     g = sign(out - y) / N, partial |err| (torch's sign: 0 at err == 0), as
//                   head_loss_kernel's loss_mode 1                  (run.py:124, :161-163 nn.L1Loss)
//   KAN_HEAD_GIVEN  g is read from yg (dLoss/dout of a loss computed elsewhere, zero on pad rows):
//                   the backward half alone -- no out, g or loss partial is written.  Same block
//                   partition and accumulation order, so fed an MSE pass's g it reproduces that
//                   pass's Gin and slab bit for bit.
template <int SRC>
__global__ __launch_bounds__(256) void kan_head_train_kernel(const float* __restrict__ X, const float* __restrict__ grid,
                                                             const float* __restrict__ W, const float* __restrict__ yg,
                                                             int64_t N, int in, int64_t n_valid, float gfac,
                                                             int64_t rows_per_block, float* __restrict__ out,
                                                             float* __restrict__ g, float* __restrict__ sse_part,
                                                             float* __restrict__ slab, float* __restrict__ Gin) {
  constexpr bool GIVEN = SRC == KAN_HEAD_GIVEN;
  __shared__ float gk[64][KF_GST];
  __shared__ float inv[64][KF_VST];
  __shared__ float part[4][KAN_K1][64];
  __shared__ float sse_w[4];
  const KanHeadLane w = kan_head_setup(gk, inv, grid, W, in);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t nb = (int64_t)blockIdx.x * rows_per_block;
  const int64_t ne = nb + rows_per_block < N ? nb + rows_per_block : N;
  const int64_t nyg = GIVEN ? ne : n_valid;  // rows whose yg is read: a given g covers the pad rows
  const bool on = lane < in;
  float ab = 0.f, as[KAN_NB] = {}, sse = 0.f;
  // the next row's x and y (or g) are loaded before this row's stores: vmcnt retires loads and
  // stores in issue order, so a load issued after the stores would wait for them too
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
    float sl, dsl, b[KAN_NB], db[KAN_NB];
    const float v = kan_head_row<true>(on, xc, gk[lane], inv[lane], w, sl, dsl, b, db);
    const KanHeadG hg = kan_head_g<SRC>(v, yc, n < n_valid, gfac, sse);
    const float gn = hg.gn;
    sse = hg.sse;
    if (!GIVEN && lane == 0) {
      out[n] = hg.o;
      g[n] = gn;
    }
    if (on) {
      ab += gn * sl;
      float d = dsl * w.wb;
#pragma unroll
      for (int c = 0; c < KAN_NB; ++c) {
        as[c] += gn * b[c];
        d += db[c] * w.ws[c];
      }
      Gin[n * in + lane] = gn * d;
    }
  }
  part[wv][0][lane] = ab;
#pragma unroll
  for (int c = 0; c < KAN_NB; ++c) part[wv][1 + c][lane] = as[c];
  if (!GIVEN && lane == 0) sse_w[wv] = sse;
  __syncthreads();
  if (wv == 0) {
    if (on) {
      float* row = slab + (int64_t)blockIdx.x * KAN_K1 * in;
#pragma unroll
      for (int t = 0; t < KAN_K1; ++t) {
        const float v = ((part[0][t][lane] + part[1][t][lane]) + part[2][t][lane]) + part[3][t][lane];
        row[t == 0 ? lane : in + KAN_NB * lane + (t - 1)] = v;
      }
    }
    if (!GIVEN && lane == 0) sse_part[blockIdx.x] = kan_head_sse(sse_w);
  }
}

// slab[z][o][k] = sum over rows of split z of G[n][o] A[n][k], for the chunk's columns k.
// 1-D grid of nchunk * nout * zpad blocks (kf_split_block).  Wave w: outs 16w .. 16w+15 x the
// chunk's kpad columns (kpad/16 accumulators), K = rows.
__global__ __launch_bounds__(256) void kan_dw_fused_kernel(const float* __restrict__ X, const float* __restrict__ grid,
                                                           const float* __restrict__ G, int64_t N, int in, int out,
                                                           int64_t rows_per_split, int nchunk, int nout, int splits,
                                                           float* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) float As[KF_KC][KF_CST];  // [kk][r]
  __shared__ __attribute__((aligned(16))) float Gt[KF_O][KF_CST];   // [o][r]
  __shared__ float Xs[KF_R][KF_IC + 1];
  __shared__ float gk[KF_IC][KF_GST];
  int cid, z;
  kf_split_block(nchunk * nout, cid, z);
  if (z >= splits) return;  // whole block, before any barrier
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const int o0 = (cid / nchunk) * KF_O;
  const KfChunk ch = kf_chunk((cid % nchunk) * KF_IC, in);
  kf_fill_knots(gk, grid, ch.i0, ch.ic);
  const int64_t rb = (int64_t)z * rows_per_split;
  const int64_t re = rb + rows_per_split < N ? rb + rows_per_split : N;
  f32x4 acc[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t r0 = rb; r0 < re; r0 += KF_R) {
    kf_stage_x(Xs, X, re, in, r0, ch.i0, ch.ic);
    if ((out & 3) == 0 && o0 + KF_O <= out) {
      KfGRegs<256> v;
      kf_g_load<256, true>(v, G, re, out, r0, o0);
      kf_g_store<256, true, true>(&Gt[0][0], v);
    } else {
      kf_g_scalar<256, false, true>(&Gt[0][0], G, re, out, r0, o0);
    }
    __syncthreads();
    kf_fill_a(As, Xs, gk, re, r0, ch);
    __syncthreads();
    if ((KAN_ABL & 2) == 0)
      kf_mfma_groups_n(ch.nkt, &Gt[16 * wv + li][4 * lk], &As[li][4 * lk], 16 * KF_CST, KF_R / 16, acc);
    __syncthreads();
  }
  kf_store_slab(slab, z, acc, ch.nkt, li, o0 + 16 * wv + 4 * lk, ch, in, out);
}

// Gin[n][i] = SiLU'(x) dA[n][i] + sum_c B'_c(x) dA[n][in + 8 i + c], dA = Gout W (never stored;
// W is read through its transposed copy WT[k][o], written by kan_combine);
// grid ceil(N/64): a block takes 64 rows through every input chunk (its Gout rows stay in LDS
// when out <= 64).  Wave w: rows 16w .. 16w+15 x the chunk's columns (kpad/16 accumulators),
// K = outs; the dA tile then goes to LDS (over the W chunk) for the contraction with the bases'
// derivatives, whose results leave through the X tile as coalesced row segments (kf_da_to_gin).
__global__ __launch_bounds__(256) void kan_dx_fused_kernel(const float* __restrict__ X, const float* __restrict__ grid,
                                                           const float* __restrict__ Gout, const float* __restrict__ WT,
                                                           int64_t N, int in, int out, float* __restrict__ Gin) {
  __shared__ __attribute__((aligned(16))) float Gs[KF_R][KF_CST];   // [r][o]
  __shared__ __attribute__((aligned(16))) float WD[KF_KC * KF_CST];  // Wt[kk][o], then dAs[r][kk]
  __shared__ float Xs[KF_R][KF_IC + 1];
  __shared__ float gk[KF_IC][KF_GST];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * KF_R;
  const bool g_once = out <= KF_O;
  for (int i0 = 0; i0 < in; i0 += KF_IC) {
    const KfChunk ch = kf_chunk(i0, in);
    f32x4 acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    kf_fill_knots(gk, grid, i0, ch.ic);
    kf_stage_x(Xs, X, N, in, r0, i0, ch.ic);
    for (int oc = 0; oc < out; oc += KF_O) {
      const int on = out - oc < KF_O ? out - oc : KF_O, opad = (on + 15) & ~15;
      const bool vec = (out & 3) == 0 && on == KF_O;
      if (!g_once || i0 == 0) {
        if (vec) {
          KfGRegs<256> v;
          kf_g_load<256, false>(v, Gout, N, out, r0, oc);
          kf_g_store<256, false, false>(&Gs[0][0], v);
        } else {
          kf_g_scalar<256, false, false>(&Gs[0][0], Gout, N, out, r0, oc);
        }
      }
      kf_load_wt<256>(WD, WT, ch, in, out, oc, vec && ch.ic == KF_IC && (in & 3) == 0);
      __syncthreads();
      if ((KAN_ABL & 2) == 0)
        kf_mfma_groups_n(ch.nkt, &Gs[16 * wv + li][4 * lk], &WD[li * KF_CST + 4 * lk], 16 * KF_CST, opad >> 4, acc);
      __syncthreads();
    }
    kf_da_to_gin<256, false>(WD, Xs, gk, acc, ch.nkt, 16 * wv + 4 * lk, li, N, r0, in, ch, nullptr, nullptr, Gin);
    __syncthreads();  // Xs / gk / WD are refilled by the next chunk
  }
}

// ---- hidden layer backward in one pass (out <= 64) --------------------------------------------
// dW and dX of a layer share the bases of every (row, input) pair and the G rows; evaluating them
// once per pass halves the recursion (with its derivative) and the G reads of kan_dw_fused +
// kan_dx_fused.  1-D grid of nchunk x zpad blocks (XCD-grouped as kan_dw_fused), 512 threads:
// a block takes one 16-input chunk and walks the 64-row tiles of its row split:
//   X, G tile -> LDS (the next tile's loads are issued before this tile's products)
//   bases + derivatives -> As[kk][r] (derivatives stay in the registers of the pair's thread)
//   dW chunk += G^T A                    (acc_w; waves: 4 out groups x 2 column halves)
//   dA = G W_chunk (W chunk resident)    (acc_x; waves: 4 row groups x 2 column halves)
//   dA -> LDS over As; Gin = SiLU' dA_base + sum_c B'_c dA_c, out through the X tile.
constexpr int KB_THREADS = 512;

__global__ __launch_bounds__(KB_THREADS) void kan_bwd_fused_kernel(const float* __restrict__ X,
                                                                  const float* __restrict__ grid,
                                                                  const float* __restrict__ G,
                                                                  const float* __restrict__ WT, int64_t N, int in,
                                                                  int out, int64_t rows_per_split, int nchunk,
                                                                  int splits, float* __restrict__ slab,
                                                                  float* __restrict__ Gin) {
  __shared__ __attribute__((aligned(16))) float AD[KF_KC * KF_CST];  // As[kk][r], then dAs[r][kk]
  __shared__ __attribute__((aligned(16))) float GG[KF_O * KF_CST];   // Gt[o][r], then Gs[r][o]
  __shared__ __attribute__((aligned(16))) float Wt[KF_KC * KF_CST];  // W chunk [kk][o]
  __shared__ float Xs[KF_R][KF_IC + 1];
  __shared__ float gk[KF_IC][KF_GST];
  int cid, z;
  kf_split_block(nchunk, cid, z);
  if (z >= splits) return;  // whole block, before any barrier
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int wr = wv & 3, wh = wv >> 2;  // 16-row (or 16-out) group, column half
  const KfChunk ch = kf_chunk(cid * KF_IC, in);
  const int j0 = 5 * wh, nj = ch.nkt - j0 < 0 ? 0 : (ch.nkt - j0 > 5 ? 5 : ch.nkt - j0);
  const int opad = (out + 15) & ~15;
  const bool vec = ch.ic == KF_IC && (in & 3) == 0 && out == KF_O;
  kf_fill_knots(gk, grid, ch.i0, ch.ic);
  // the chunk's W^T [kk][o] stays in LDS for the whole split
  kf_load_wt<KB_THREADS>(Wt, WT, ch, in, out, 0, false);
  const int64_t rb = (int64_t)z * rows_per_split;
  const int64_t re = rb + rows_per_split < N ? rb + rows_per_split : N;
  f32x4 accw[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) accw[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // tile loads (vec path): X one float4 for threads < 256, G two float4 per thread
  const int xr = tid >> 2, xi = (tid & 3) * 4;
  auto load_x = [&](int64_t r0) {
    float4 v = float4{0.f, 0.f, 0.f, 0.f};
    if (tid < 256 && r0 + xr < re) v = ldg4(X + (r0 + xr) * in + ch.i0 + xi);
    return v;
  };
  float4 xv = float4{0.f, 0.f, 0.f, 0.f};
  KfGRegs<KB_THREADS> gv = {xv, xv};
  if (vec && rb < re) {
    xv = load_x(rb);
    kf_g_load<KB_THREADS, true>(gv, G, re, out, rb, 0);
  }
  for (int64_t r0 = rb; r0 < re; r0 += KF_R) {
    // ---- X and G^T tiles into LDS
    if (vec) {
      if (tid < 256) {
        Xs[xr][xi] = xv.x;
        Xs[xr][xi + 1] = xv.y;
        Xs[xr][xi + 2] = xv.z;
        Xs[xr][xi + 3] = xv.w;
      }
      kf_g_store<KB_THREADS, true, true>(GG, gv);
    } else {
      kf_stage_x(Xs, X, re, in, r0, ch.i0, ch.ic);
      kf_g_scalar<KB_THREADS, true, true>(GG, G, re, out, r0, 0);
    }
    __syncthreads();
    // ---- bases (As) and derivatives (registers) of the thread's pairs
    float dsl[2], dbs[2][KAN_NB];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int p = tid + KB_THREADS * h, r = p & 63, ii = p >> 6;
      dsl[h] = 0.f;
#pragma unroll
      for (int c = 0; c < KAN_NB; ++c) dbs[h][c] = 0.f;
      if (ii < ch.ic) {
        float b[KAN_NB], sl = 0.f;
#pragma unroll
        for (int c = 0; c < KAN_NB; ++c) b[c] = 0.f;
        if (r0 + r < re) {
          const float x = Xs[r][ii];
          kan_bases_local<true, true>(x, gk[ii], b, dbs[h]);
          silu_and_grad(x, sl, dsl[h]);
        }
        AD[ii * KF_CST + r] = sl;
#pragma unroll
        for (int c = 0; c < KAN_NB; ++c) AD[(ch.ic + 8 * ii + c) * KF_CST + r] = b[c];
      }
    }
    for (int e = tid; e < (ch.kpad - ch.kc) * KF_R; e += KB_THREADS) AD[(ch.kc + e / KF_R) * KF_CST + e % KF_R] = 0.f;
    __syncthreads();
    // ---- the next tile's loads go out under this tile's products
    float4 nxv = xv;
    KfGRegs<KB_THREADS> ngv = {gv[0], gv[1]};
    if (vec && r0 + KF_R < re) {
      nxv = load_x(r0 + KF_R);
      kf_g_load<KB_THREADS, true>(ngv, G, re, out, r0 + KF_R, 0);
    }
    // ---- dW chunk += G^T A over the tile's rows
    if ((KAN_ABL & 2) == 0)
      kf_mfma_groups_n(nj, &GG[(16 * wr + li) * KF_CST + 4 * lk], &AD[(16 * j0 + li) * KF_CST + 4 * lk], 16 * KF_CST,
                       KF_R / 16, accw);
    __syncthreads();
    // ---- G rows [r][o] over G^T, then dA = G W_chunk
    if (vec) kf_g_store<KB_THREADS, true, false>(GG, gv);
    else kf_g_scalar<KB_THREADS, false, false>(GG, G, re, out, r0, 0);
    __syncthreads();
    f32x4 accx[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) accx[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if ((KAN_ABL & 2) == 0)
      kf_mfma_groups_n(nj, &GG[(16 * wr + li) * KF_CST + 4 * lk], &Wt[(16 * j0 + li) * KF_CST + 4 * lk], 16 * KF_CST,
                       opad >> 4, accx);
    // ---- dA over As (last read by the dW products, before the barrier above), Gin through the X tile
    kf_da_to_gin<KB_THREADS, true>(AD, Xs, gk, accx, nj, 16 * wr + 4 * lk, 16 * j0 + li, re, r0, in, ch, dsl, dbs, Gin);
    xv = nxv;
    gv[0] = ngv[0];
    gv[1] = ngv[1];
    __syncthreads();  // Xs / GG / AD are refilled by the next tile
  }
  kf_store_slab(slab, z, accw, nj, 16 * j0 + li, 16 * wr + 4 * lk, ch, in, out);
}

// ---- strided fp32 GEMM:  C[m][n] = sum_k A(m, k) B(k, n) --------------------------------
// A(m, k) = A[m*sam + k*sak], B(k, n) = B[k*sbk + n*sbn]; 64x64 tile, BK 16, 256 threads,
// 4x4 outputs per thread; split-K over blockIdx.z writes slab z of C (C + z*M*N) which
// kan_slab_reduce sums in fixed order.  Bounds-checked (zero fill) for any M, N, K.
constexpr int KG_T = 64, KG_BK = 16;

__global__ __launch_bounds__(256) void kan_gemm_kernel(const float* __restrict__ A, int64_t sam, int64_t sak,
                                                       const float* __restrict__ B, int64_t sbk, int64_t sbn,
                                                       float* __restrict__ C, int M, int N, int64_t K,
                                                       int64_t kchunk) {
  __shared__ float As[KG_BK][KG_T + 4];
  __shared__ float Bs[KG_BK][KG_T + 4];
  const int tid = threadIdx.x;
  const int m0 = blockIdx.y * KG_T, n0 = blockIdx.x * KG_T;
  const int64_t kb = (int64_t)blockIdx.z * kchunk;
  const int64_t ke = (kb + kchunk < K) ? kb + kchunk : K;
  C += (int64_t)blockIdx.z * M * N;
  const int tm = (tid / 16) * 4, tn = (tid % 16) * 4;
  float acc[4][4] = {};
  // loader index -> (k, m) with the unit-stride dimension fastest across threads (coalesced)
  const bool a_k_fast = (sak == 1), b_k_fast = (sbk == 1);
  for (int64_t k0 = kb; k0 < ke; k0 += KG_BK) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int idx = tid + r * 256;
      int kk, mm;
      if (a_k_fast) { kk = idx % KG_BK; mm = idx / KG_BK; } else { kk = idx / KG_T; mm = idx % KG_T; }
      const int64_t k = k0 + kk;
      const int m = m0 + mm;
      As[kk][mm] = (k < ke && m < M) ? A[(int64_t)m * sam + k * sak] : 0.f;
      int nn;
      if (b_k_fast) { kk = idx % KG_BK; nn = idx / KG_BK; } else { kk = idx / KG_T; nn = idx % KG_T; }
      const int64_t kq = k0 + kk;
      const int n = n0 + nn;
      Bs[kk][nn] = (kq < ke && n < N) ? B[kq * sbk + (int64_t)n * sbn] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KG_BK; ++kk) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[kk][tm + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Bs[kk][tn + j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + tm + i, n = n0 + tn + j;
      if (m < M && n < N) C[(int64_t)m * N + n] = acc[i][j];
    }
}

// ---- the grid-5 launchers (declared in kan_tiles.h; the entry points of siren_kernels.h, in
// kan_general.hip, check the shapes and pick the set) ----------------------------------------
hipError_t kan5_fwd_fused(const float* X, const float* grid, const float* W, int64_t N, int in, int out, float* Y,
                          hipStream_t s) {
  hipLaunchKernelGGL(kan_fwd_fused_kernel, dim3((unsigned)((N + KF_R - 1) / KF_R), (out + KF_O - 1) / KF_O), dim3(256),
                     0, s, X, grid, W, N, in, out, Y);
  return hipGetLastError();
}

hipError_t kan5_head_fwd(const float* X, const float* grid, const float* W, int64_t N, int in, float* Y, hipStream_t s) {
  const int64_t blocks = (N + 3) / 4;
  hipLaunchKernelGGL(kan_head_fwd_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, s, X, grid, W,
                     N, in, Y);
  return hipGetLastError();
}

template <int SRC>
static void kan5_head_launch(const KanHeadPlan& p, const float* X, const float* grid, const float* W, const float* yg,
                             int64_t N, int in, int64_t n_valid, float gfac, float* out, float* g, float* sse_part,
                             float* slab, float* Gin, hipStream_t s) {
  hipLaunchKernelGGL(kan_head_train_kernel<SRC>, dim3(p.blocks), dim3(256), 0, s, X, grid, W, yg, N, in, n_valid, gfac,
                     p.rows_per_block, out, g, sse_part, slab, Gin);
}

// the head pass over kan_head_plan's blocks for g from src (KAN_HEAD_*); the caller sums the slab
hipError_t kan5_head_pass(int src, const KanHeadPlan& p, const float* X, const float* grid, const float* W,
                          const float* yg, int64_t N, int in, int64_t n_valid, float gfac, float* out, float* g,
                          float* sse_part, float* slab, float* Gin, hipStream_t s) {
  (src == KAN_HEAD_GIVEN ? kan5_head_launch<KAN_HEAD_GIVEN>
   : src == KAN_HEAD_L1  ? kan5_head_launch<KAN_HEAD_L1>
                         : kan5_head_launch<KAN_HEAD_MSE>)(p, X, grid, W, yg, N, in, n_valid, gfac, out, g, sse_part,
                                                           slab, Gin, s);
  return hipGetLastError();
}

// slab[z] of dW[o][k] = sum_n G[n][o] A[n][k] over the plan's row splits
hipError_t kan5_dw_fused(const KfDwPlan& p, const float* X, const float* grid, const float* G, int64_t N, int in,
                         int out, float* slab, hipStream_t s) {
  hipLaunchKernelGGL(kan_dw_fused_kernel, dim3(p.split.blocks), dim3(256), 0, s, X, grid, G, N, in, out,
                     p.split.rows_per_split, p.nchunk, p.nout, p.split.z, slab);
  return hipGetLastError();
}

hipError_t kan5_dx_fused(const float* X, const float* grid, const float* Gout, const float* WT, int64_t N, int in,
                         int out, float* Gin, hipStream_t s) {
  hipLaunchKernelGGL(kan_dx_fused_kernel, dim3((unsigned)((N + KF_R - 1) / KF_R)), dim3(256), 0, s, X, grid, Gout, WT,
                     N, in, out, Gin);
  return hipGetLastError();
}

// dW (split-K slabs + fixed-order sum) and Gin of a layer with out <= 64 in one pass
hipError_t kan5_bwd_fused(const float* X, const float* grid, const float* G, const float* WT, int64_t N, int in,
                          int out, int64_t max_splits, float* slab, float* dW, float* Gin, hipStream_t s) {
  if (out > KF_O) return hipErrorInvalidValue;
  const int nchunk = (in + KF_IC - 1) / KF_IC;
  const KfSplitPlan p = kf_plan_splits(N, kKanBwdResidentBlocks, nchunk, max_splits);
  if (!p.blocks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kan_bwd_fused_kernel, dim3(p.blocks), dim3(KB_THREADS), 0, s, X, grid, G, WT, N, in, out,
                     p.rows_per_split, nchunk, p.z, slab, Gin);
  return slab_reduce(slab, p.z, (int64_t)out * KAN_K1 * in, dW, s);
}

// splits > 1: `C` must hold splits * M * N floats (slabs), reduced into `out`
hipError_t kan_gemm(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, int M,
                    int N, int64_t K, int splits, float* C, float* out, hipStream_t s) {
  if (M <= 0 || N <= 0 || K <= 0 || splits < 1) return hipErrorInvalidValue;
  int64_t kchunk = (K + splits - 1) / splits;
  kchunk = (kchunk + KG_BK - 1) / KG_BK * KG_BK;
  const int z = (int)((K + kchunk - 1) / kchunk);
  dim3 grid((N + KG_T - 1) / KG_T, (M + KG_T - 1) / KG_T, z);
  hipLaunchKernelGGL(kan_gemm_kernel, grid, dim3(256), 0, s, A, sam, sak, B, sbk, sbn, z > 1 ? C : out, M, N, K,
                     kchunk);
  if (z > 1) return slab_reduce(C, z, (int64_t)M * N, out, s);
  return hipGetLastError();
}


}  // namespace siren
