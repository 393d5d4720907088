// Gaussian random-Fourier-feature input encoding (run.py:141-144, rff.layers.GaussianEncoding):
//   enc(x)[j] = cos(2 pi x B[j]),  enc(x)[F + j] = sin(2 pi x B[j]),  j < F,  x [rows][1], B [F][1]
// feeding net.0 = SineLayer(2F, H, is_first, omega0) or (first_linear) Linear(2F, H) + Snake.
//
// rff_first_fwd: the encoded first layer in one launch.  A block owns a 128-row x 128-column
// tile and walks K = 2F in steps of 32.  Per step the 256 threads build the A operand in LDS
// from x and B (16 elements each: thread = one encoding column, 16 rows) and stage the matching
// 128 x 32 piece of W0 (prefetched into registers under the previous step's MFMAs); the fp32
// [rows][2F] matrix never exists in memory.  The product is exact fp32 on
// v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain): fp16 operands would move the pre-activation
// by ~0.08 rad at omega0 = 22000.  Column tile 0 also writes enc once as fp16 [rows][KP] for the
// weight gradient (fp16 MFMA operands there, like every other dW of the project).
//
// LDS map (36 864 B per block, 4 blocks per CU):
//   As [128 rows][36] fp32  18 432 B   enc chunk, row stride 32 + 4 floats
//   Ws [128 cols][36] fp32  18 432 B   W0 chunk
// Fragment reads are one ds_read_b128 per 16-row subtile and 16-k half: lane l takes elements
// 4 (l >> 4) .. + 3 of row l & 15 and uses element s as its operand of MFMA s.  The instruction
// wants k = l >> 4; taking k = 4 (l >> 4) + s for BOTH operands is a permutation of the sum's
// terms inside a 16-k group, and the 4-float row padding keeps the 16 rows of a read on distinct
// bank groups.  The operand roles are swapped (A := W0 rows, B := enc rows) so a lane holds 4
// consecutive output columns of one row; adjacent column subtiles are exchanged with
// swap16_pair and Y0 / C0 / E0 leave as 16-B row pieces (as gemm_nt.hip).
//
// The argument is reduced in revolutions before v_cos_f32 / v_sin_f32, as the existing first
// layer does: p = x b rounded, e = fma(x, b, -p) its exact residual, r = (p - rint p) + e, so r
// is x b mod 1 to ~2^-25 revolutions whatever |x b| is.
//
// Backward (capi.hip run_backward): gemm_nt's NT_DX / NT_DX_SNAKE epilogue stores
// cos (dZ1 W1) S without omega0 (omega0 cos (dZ W) S overflows fp16 at the S chosen for hidden
// layers whose omega is 30); gemm_tn_dw forms dZ0^T enc split-K over the rows on 128 x 128 tiles,
// dw_reduce sums the slices (x 1/S), and rff_dw0_finish applies omega0 in fp32 while it
// accumulates the [H][2F] block of the [H][KP] result into the gradient.
#include "siren_common.h"
#include "siren_kernels.h"

namespace siren {

namespace {

constexpr int RF_BM = 128, RF_BN = 128, RF_BK = 32, RF_LD = RF_BK + 4, RF_THREADS = 256;

// cos / sin of 2 pi x b with the product reduced exactly in revolutions
__device__ __forceinline__ float rff_phase(float x, float b) {
  const float p = x * b;
  const float e = __builtin_fmaf(x, b, -p);  // exact: x b = p + e
  return (p - __builtin_rintf(p)) + e;
}
__device__ __forceinline__ float rff_enc(float x, float b, bool is_sin) {
  const float r = rff_phase(x, b);
  return is_sin ? __builtin_amdgcn_sinf(r) : __builtin_amdgcn_cosf(r);
}

__device__ __forceinline__ f32x4 rf_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <bool SNAKE>
__global__ __launch_bounds__(RF_THREADS) void rff_first_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ Bf, int F, const float* __restrict__ W0,
    const float* __restrict__ b0, float omega0, int H, h16* __restrict__ Y0, h16* __restrict__ C0,
    const float* __restrict__ a0, h16* __restrict__ E0, h16* __restrict__ enc, int KP) {
  __shared__ __attribute__((aligned(16))) float As[RF_BM][RF_LD];
  __shared__ __attribute__((aligned(16))) float Ws[RF_BN][RF_LD];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nct = H / RF_BN;
  const int rt = blockIdx.x / nct, ct = blockIdx.x - rt * nct;
  const int r0 = rt * RF_BM, c0 = ct * RF_BN;
  const int K2 = 2 * F, nk = (K2 + RF_BK - 1) / RF_BK;
  const bool put_enc = enc != nullptr && ct == 0;

  // staging role: encoding column sk of the step, rows / W0 rows sr + 8 i
  const int sk = tid & 31, sr = tid >> 5;
  float xr[16], wnx[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) xr[i] = x[r0 + sr + 8 * i];
  auto load_b = [&](int kc) {
    const int kk = kc * RF_BK + sk;
    return kk < K2 ? Bf[kk < F ? kk : kk - F] : 0.f;
  };
  auto load_w = [&](int kc) {
    const int kk = kc * RF_BK + sk;
#pragma unroll
    for (int i = 0; i < 16; ++i) wnx[i] = kk < K2 ? W0[(size_t)(c0 + sr + 8 * i) * K2 + kk] : 0.f;
  };
  float bj = load_b(0);
  load_w(0);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fk = 4 * (lane >> 4);
  for (int kc = 0; kc < nk; ++kc) {
    const int kk = kc * RF_BK + sk;
    const bool valid = kk < K2, is_sin = kk >= F;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float v = valid ? rff_enc(xr[i], bj, is_sin) : 0.f;
      As[sr + 8 * i][sk] = v;
      Ws[sr + 8 * i][sk] = wnx[i];
      if (put_enc) enc[(size_t)(r0 + sr + 8 * i) * KP + kk] = (h16)v;
    }
    if (kc + 1 < nk) {  // the next step's B and W0 piece travel under this step's MFMAs
      bj = load_b(kc + 1);
      load_w(kc + 1);
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < RF_BK / 16; ++h) {
      float4 af[4], wf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = *(const float4*)&As[wm * 64 + i * 16 + fr][16 * h + fk];
#pragma unroll
      for (int j = 0; j < 4; ++j) wf[j] = *(const float4*)&Ws[wn * 64 + j * 16 + fr][16 * h + fk];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[i][j] = rf_mfma(wf[j].x, af[i].x, acc[i][j]);
          acc[i][j] = rf_mfma(wf[j].y, af[i].y, acc[i][j]);
          acc[i][j] = rf_mfma(wf[j].z, af[i].z, acc[i][j]);
          acc[i][j] = rf_mfma(wf[j].w, af[i].w, acc[i][j]);
        }
    }
    __syncthreads();
  }
  if (put_enc) {  // the rest of the padded row: zero operand columns of the weight-gradient GEMM
    for (int kk = nk * RF_BK + sk; kk < KP; kk += RF_BK)
#pragma unroll
      for (int i = 0; i < 16; ++i) enc[(size_t)(r0 + sr + 8 * i) * KP + kk] = (h16)0.f;
  }

  // acc[i][j][r] = z[row r0 + wm 64 + i 16 + (lane & 15)][col c0 + wn 64 + j 16 + 4 (lane >> 4) + r]
  // the existing first layer's epilogue: a0 = omega0 (z + b0), one fp32 sincos in revolutions;
  // first_linear: Snake of z + b0
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const size_t row = (size_t)(r0 + wm * 64 + i * 16 + fr);
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
      uint2 yv[2], cv[2], ev[2];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int col = c0 + wn * 64 + (2 * jp + jj) * 16 + fk;
        const float4 bb = *(const float4*)(b0 + col);
        const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
        float y[4], c[4], e[4];
        if constexpr (SNAKE) {
          const float4 aa = *(const float4*)(a0 + col);
          const float av[4] = {aa.x, aa.y, aa.z, aa.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) snake_epi(acc[i][2 * jp + jj][r] + bv[r], av[r], 1.0f / av[r], y[r], c[r], e[r]);
          ev[jj] = as_u2(pack4(e[0], e[1], e[2], e[3]));
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) sincos_rev(omega0 * (acc[i][2 * jp + jj][r] + bv[r]), &y[r], &c[r]);
        }
        yv[jj] = as_u2(pack4(y[0], y[1], y[2], y[3]));
        cv[jj] = as_u2(pack4(c[0], c[1], c[2], c[3]));
      }
      const size_t o = row * H + c0 + wn * 64 + jp * 32 + swap16_col(lane);
      *(uint4*)(Y0 + o) = swap16_pair(yv[0], yv[1]);
      *(uint4*)(C0 + o) = swap16_pair(cv[0], cv[1]);
      if constexpr (SNAKE) *(uint4*)(E0 + o) = swap16_pair(ev[0], ev[1]);
    }
  }
}

// enc as fp16 [rows][KP] (columns 2F .. KP-1 zero): the stand-alone backward's copy of what the
// forward's column tile 0 writes (the same values: the same rff_enc)
__global__ void rff_encode16_kernel(const float* __restrict__ x, const float* __restrict__ Bf, int F, int64_t rows,
                                    int KP, h16* __restrict__ enc) {
  const int64_t total = rows * KP;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = q / KP;
    const int kk = (int)(q - r * KP);
    enc[q] = kk < 2 * F ? (h16)rff_enc(x[r], Bf[kk < F ? kk : kk - F], kk >= F) : (h16)0.f;
  }
}

// the module API's encoding: fp32 [rows][2F]
__global__ void rff_encode_kernel(const float* __restrict__ x, const float* __restrict__ Bf, int F, int64_t rows,
                                  float* __restrict__ out) {
  const int K2 = 2 * F;
  const int64_t total = rows * K2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = q / K2;
    const int kk = (int)(q - r * K2);
    out[q] = rff_enc(x[r], Bf[kk < F ? kk : kk - F], kk >= F);
  }
}

// gW0[h][j] += scale dW[h][j] (dW [H][KP], j < 2F) and, db != null, gb0[h] += scale db[h]
__global__ void rff_dw0_finish_kernel(const float* __restrict__ dW, int H, int K2, int KP, float scale,
                                      float* __restrict__ gW0, const float* __restrict__ db, float* __restrict__ gb0) {
  const int total = H * K2;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < total; q += gridDim.x * blockDim.x) {
    const int h = q / K2, j = q - h * K2;
    gW0[q] += scale * dW[(size_t)h * KP + j];
    if (db != nullptr && j == 0) gb0[h] += scale * db[h];
  }
}

int grid_1d(int64_t total, int block, int cap) {
  const int64_t g = (total + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

int rff_kpad(int F) { return (2 * F + 127) / 128 * 128; }

int rff_splits(int R, int H, int F) {
  // 128 x 128 tiles (the one tile shape every H and KP takes): ~1024 blocks, no slice thinner
  // than 8 K-steps of 64 rows (as siren_default_splits)
  const int ntile = (rff_kpad(F) / 128) * (H / 128);
  int splits = 1024 / (ntile > 0 ? ntile : 1);
  const int max_splits = R / 64 / 8 > 0 ? R / 64 / 8 : 1;
  if (splits > max_splits) splits = max_splits;
  return splits < 1 ? 1 : splits;
}

int64_t rff_slab_floats(int R, int H, int F) {
  return ((int64_t)rff_splits(R, H, F) + 1) * H * rff_kpad(F) + H;
}

hipError_t rff_encode(const float* x, const float* Bf, int F, int64_t rows, float* out, hipStream_t s) {
  if (F < 1 || F > kRffMaxFreq || rows < 0) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(rff_encode_kernel, dim3(grid_1d(rows * 2 * F, 256, 8192)), dim3(256), 0, s, x, Bf, F, rows, out);
  return hipGetLastError();
}

hipError_t rff_encode16(const float* x, const float* Bf, int F, int R, h16* enc, hipStream_t s) {
  if (F < 1 || F > kRffMaxFreq || R <= 0) return hipErrorInvalidValue;
  const int KP = rff_kpad(F);
  hipLaunchKernelGGL(rff_encode16_kernel, dim3(grid_1d((int64_t)R * KP, 256, 8192)), dim3(256), 0, s, x, Bf, F,
                     (int64_t)R, KP, enc);
  return hipGetLastError();
}

hipError_t rff_first_fwd(const float* x, const float* Bf, int F, const float* W0, const float* b0, float omega0, int R,
                         int H, h16* Y0, h16* C0, const float* a0, h16* E0, h16* enc, hipStream_t s) {
  if (F < 1 || F > kRffMaxFreq || R <= 0 || R % RF_BM || H <= 0 || H % RF_BN) return hipErrorInvalidValue;
  if ((a0 != nullptr) != (E0 != nullptr)) return hipErrorInvalidValue;
  const int64_t blocks = (int64_t)(R / RF_BM) * (H / RF_BN);
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  const int KP = rff_kpad(F);
  if (a0)
    hipLaunchKernelGGL(rff_first_fwd_kernel<true>, dim3((unsigned)blocks), dim3(RF_THREADS), 0, s, x, Bf, F, W0, b0,
                       omega0, H, Y0, C0, a0, E0, enc, KP);
  else
    hipLaunchKernelGGL(rff_first_fwd_kernel<false>, dim3((unsigned)blocks), dim3(RF_THREADS), 0, s, x, Bf, F, W0, b0,
                       omega0, H, Y0, C0, a0, E0, enc, KP);
  return hipGetLastError();
}

hipError_t rff_dw0(const h16* enc, const h16* dZ0, int F, int R, int H, float scale, const float* gscale,
                   float* slab, const float* db, float* gW0, float* gb0, hipStream_t s) {
  if (F < 1 || F > kRffMaxFreq || R <= 0 || R % 64 || H % 128) return hipErrorInvalidValue;
  const int KP = rff_kpad(F), splits = rff_splits(R, H, F);
  TnParams tp = {};
  tp.Y = enc; tp.dZ = dZ0;
  tp.R = R; tp.Hin = KP; tp.Hout = H;
  tp.splits = splits;
  tp.tile = 128;
  tp.slab = slab;
  hipError_t e = gemm_tn_dw(tp, s);
  if (e != hipSuccess) return e;
  float* dW = slab + (size_t)splits * H * KP;  // [H][KP], x 1/S
  e = dw_reduce(slab, splits, KP, H, 128, dW, 0, gscale, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rff_dw0_finish_kernel, dim3(grid_1d((int64_t)H * 2 * F, 256, 4096)), dim3(256), 0, s, dW, H, 2 * F,
                     KP, scale, gW0, db, gb0);
  return hipGetLastError();
}

}  // namespace siren
