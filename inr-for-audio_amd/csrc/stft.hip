// STFT and SNR losses (run.py:126-128, :160-169: auraloss.freq.STFTLoss() and
// auraloss.time.SNRLoss(), restated from their published 0.4.0 definitions) and the loss mix
//   loss = (1 - alpha) {L1 | L_snr | MSE} + alpha L_stft
// for the model output x and the target y, both one sequence of n samples.
//
//   X = stft(x, n_fft 1024, hop 256, periodic Hann, center, reflect)   T = 1 + n / 256 frames, 513 bins
//   x_mag = sqrt(max(re^2 + im^2, 1e-8))
//   L_stft = ||y_mag - x_mag||_F / ||y_mag||_F + mean |log x_mag - log y_mag|
//   L_snr  = -10 log10(sum yc^2 / (sum (xc - yc)^2 + 1e-8) + 1e-8),  xc = x - mean x, yc = y - mean y
//
// The transform is a GEMM against windowed cos / -sin tables (fp64 on the host, rounded to fp32 once)
// on v_mfma_f32_16x16x4_f32: a small bin's log amplifies its error by 1 / x_mag, so no fp16 operands.
//
// stft_fwd_kernel: a block owns 16 frames and 12 bin tiles of 16 (3 per wave; grid.y 3 covers the
// 33 tiles of the 528 padded bins).  The 16 overlapping frames are read from the signal itself: the
// 15 * 256 + 1024 = 4864 padded samples they span are staged once in LDS (reflection folded in the
// staging index), never as a [T][1024] matrix.
//   LDS map: sig[4940] fp32 (19 760 B): padded sample q of the tile at q + 4 (q >> 8)
// Frame f starts at q = 256 f, so without the skew the 16 rows of one ds_read_b128 fragment would
// be 256 floats apart -- one bank for all of them; with it they are 260 apart, i.e. 4 banks each,
// the 16 rows x 4 floats of a read covering all 64 banks once.  A float4 never straddles a multiple
// of 256, so it stays contiguous and 16-B aligned.
// The basis is read from global memory (L2-resident, 4.3 MB) in a fragment-native layout,
//   fwd[c][k / 16][bin][k % 16]   (c: 0 = w cos, 1 = -w sin; bin < 528, zero past 512)
// so one wave's 16 bins x 16 k piece is 1 KB contiguous.  As in rff.hip a lane takes k = 4 (l >> 4) + s
// of a 16-k group as its operand of MFMA s for both operands (a permutation of the sum's terms).
// The basis is the MFMA's A operand and the frames its B operand: a lane then holds 4 consecutive
// bins of ONE frame in both the cos and the sin accumulator, forms the magnitude without a lane
// exchange and stores re / im as 16-B pieces.  K is accumulated in two interleaved chains (even /
// odd 16-k groups), summed at the end: 512-term instead of 1024-term fma chains.
//
// stft_bwd_kernel: dF[T][1024] = [dRe | dIm][T][2 x 528] x basis^T, the table transposed to
//   bwd[c][bin / 16][k][bin % 16]
// The B operand (d of one frame, 4 consecutive bins per lane) is formed from re / im, the target's
// magnitudes and the finished scalars as it is loaded:
//   d = (x_mag - y_mag) / (sqrt S1 sqrt Sy) + sign(log x_mag - log y_mag) / (x_mag T 513),  0 at the clamp
//   dRe = d re / x_mag, dIm = d im / x_mag
// stft_gather then sums, per sample, the <= 4 frames that cover it and the same for its reflected
// images, in a fixed order -- no float atomics anywhere, two runs are bit-identical.
#include <math.h>
#include "siren_common.h"
#include "siren_kernels.h"

namespace siren {

namespace {

constexpr int SF_N = kStftFft, SF_HOP = kStftHop, SF_NB = kStftBins, SF_NBP = kStftBinsPad;
constexpr int SF_NBT = SF_NBP / 16;                     // 33 bin tiles
constexpr int SF_KT = SF_N / 16;                        // 64 k groups
constexpr int SF_FT = 16;                               // frames per block
constexpr int SF_SEG = (SF_FT - 1) * SF_HOP + SF_N;     // 4864 padded samples per block
constexpr int SF_SEGP = SF_SEG + 4 * (SF_SEG / 256);    // + the skew
constexpr int SF_WT = 3;                                // forward: bin tiles per wave
constexpr int SF_FGY = (SF_NBT + 4 * SF_WT - 1) / (4 * SF_WT);  // forward grid.y (3)
constexpr int SF_BWT = 4;                               // backward: sample tiles per wave
constexpr int SF_BGY = SF_N / 16 / (4 * SF_BWT);        // backward grid.y (4)
constexpr float SF_EPS = 1e-8f;
constexpr size_t SF_TAB = (size_t)2 * SF_N * SF_NBP;    // floats of one table

__device__ __forceinline__ f32x4 sf_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// sample at padded index j of the centred, reflect-padded signal (0 past the padded end: frames >= T)
__device__ __forceinline__ float stft_sample(const float* __restrict__ x, int n, int64_t j) {
  int64_t i = j - SF_N / 2;
  if (i < 0) {
    i = -i;
  } else if (i >= n) {
    i = 2 * (int64_t)(n - 1) - i;
    if (i < 0) return 0.f;
  }
  return x[i];
}

template <bool TARGET>
__global__ __launch_bounds__(256) void stft_fwd_kernel(const float* __restrict__ x, int n, int T,
                                                       const float* __restrict__ basis, float* __restrict__ o0,
                                                       float* __restrict__ o1, const float* __restrict__ ymag,
                                                       const float* __restrict__ ylog, float* __restrict__ part,
                                                       int npart) {
  __shared__ __attribute__((aligned(16))) float sig[SF_SEGP];
  __shared__ float scratch[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t0 = blockIdx.x * SF_FT;
  const int64_t j0 = (int64_t)t0 * SF_HOP;
  for (int q = tid; q < SF_SEG; q += 256) sig[q + 4 * (q >> 8)] = stft_sample(x, n, j0 + q);
  __syncthreads();

  const int fr = lane & 15, fk = 4 * (lane >> 4);
  const int bt0 = (blockIdx.y * 4 + wave) * SF_WT;
  f32x4 ac[2][SF_WT], as[2][SF_WT];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < SF_WT; ++j) ac[h][j] = as[h][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto load_b = [&](int kt, float4 (&bc)[SF_WT], float4 (&bs)[SF_WT]) {
#pragma unroll
    for (int j = 0; j < SF_WT; ++j) {
      // a tile past the 33rd (the last wave of grid.y 2) re-reads tile 32: its results are not stored,
      // and without a branch here the pieces stay in registers
      const int bt = bt0 + j < SF_NBT ? bt0 + j : SF_NBT - 1;
      const size_t o = ((size_t)kt * SF_NBP + bt * 16 + fr) * 16 + fk;
      bc[j] = *(const float4*)(basis + o);
      bs[j] = *(const float4*)(basis + (size_t)SF_N * SF_NBP + o);
    }
  };
  auto step = [&](int kt, const float4 (&bc)[SF_WT], const float4 (&bs)[SF_WT], f32x4 (&c)[SF_WT],
                  f32x4 (&s)[SF_WT]) {
    const int idx = 256 * fr + 16 * kt + fk;
    const float4 a = *(const float4*)&sig[idx + 4 * (idx >> 8)];
#pragma unroll
    for (int j = 0; j < SF_WT; ++j) {
      c[j] = sf_mfma(bc[j].x, a.x, c[j]);
      s[j] = sf_mfma(bs[j].x, a.x, s[j]);
      c[j] = sf_mfma(bc[j].y, a.y, c[j]);
      s[j] = sf_mfma(bs[j].y, a.y, s[j]);
      c[j] = sf_mfma(bc[j].z, a.z, c[j]);
      s[j] = sf_mfma(bs[j].z, a.z, s[j]);
      c[j] = sf_mfma(bc[j].w, a.w, c[j]);
      s[j] = sf_mfma(bs[j].w, a.w, s[j]);
    }
  };
  // the next 16-k group's basis pieces travel under this group's MFMAs
  float4 bcA[SF_WT], bsA[SF_WT], bcB[SF_WT], bsB[SF_WT];
  load_b(0, bcA, bsA);
  for (int kt = 0; kt < SF_KT; kt += 2) {
    load_b(kt + 1, bcB, bsB);
    step(kt, bcA, bsA, ac[0], as[0]);
    if (kt + 2 < SF_KT) load_b(kt + 2, bcA, bsA);
    step(kt + 1, bcB, bsB, ac[1], as[1]);
  }

  // lane: frame t0 + fr, bins (bt0 + j) 16 + fk + r
  const int t = t0 + fr;
  float s1 = 0.f, sl = 0.f;
#pragma unroll
  for (int j = 0; j < SF_WT; ++j) {
    if (bt0 + j >= SF_NBT || t >= T) continue;
    const f32x4 re = ac[0][j] + ac[1][j], im = as[0][j] + as[1][j];
    const size_t o = (size_t)t * SF_NBP + (bt0 + j) * 16 + fk;
    float mag[4], lg[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mag[r] = sqrtf(fmaxf(re[r] * re[r] + im[r] * im[r], SF_EPS));
      lg[r] = logf(mag[r]);
    }
    if constexpr (TARGET) {
      *(float4*)(o0 + o) = float4{mag[0], mag[1], mag[2], mag[3]};
      *(float4*)(o1 + o) = float4{lg[0], lg[1], lg[2], lg[3]};
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if ((bt0 + j) * 16 + fk + r < SF_NB) s1 += mag[r] * mag[r];
    } else {
      *(float4*)(o0 + o) = float4{re[0], re[1], re[2], re[3]};
      *(float4*)(o1 + o) = float4{im[0], im[1], im[2], im[3]};
      const float4 ym = *(const float4*)(ymag + o), yl = *(const float4*)(ylog + o);
      const float ymv[4] = {ym.x, ym.y, ym.z, ym.w}, ylv[4] = {yl.x, yl.y, yl.z, yl.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if ((bt0 + j) * 16 + fk + r < SF_NB) {
          const float dm = ymv[r] - mag[r];
          s1 += dm * dm;
          sl += fabsf(lg[r] - ylv[r]);
        }
    }
  }
  s1 = block_sum(s1, scratch);
  sl = block_sum(sl, scratch);
  if (tid == 0) {
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    part[(size_t)PT_S1 * npart + blk] = s1;
    part[(size_t)PT_SL * npart + blk] = sl;
  }
}

__global__ __launch_bounds__(256) void stft_bwd_kernel(int T, const float* __restrict__ basisT,
                                                       const float* __restrict__ re, const float* __restrict__ im,
                                                       const float* __restrict__ ymag,
                                                       const float* __restrict__ ylog,
                                                       const float* __restrict__ scal, float* __restrict__ dF) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fk = 4 * (lane >> 4);
  const int t = blockIdx.x * SF_FT + fr;
  const bool valid = t < T;
  const int nt0 = (blockIdx.y * 4 + wave) * SF_BWT;
  const float c1 = scal[SC_C1], c2 = scal[SC_C2];
  f32x4 acc[2][SF_BWT];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < SF_BWT; ++j) acc[h][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  struct Raw { float4 re, im, ym, yl; };
  auto load_raw = [&](int bg, Raw& w) {
    if (valid) {
      const size_t o = (size_t)t * SF_NBP + bg * 16 + fk;
      w.re = *(const float4*)(re + o);
      w.im = *(const float4*)(im + o);
      w.ym = *(const float4*)(ymag + o);
      w.yl = *(const float4*)(ylog + o);
    }
  };
  // d of 4 consecutive bins of this lane's frame -> (dRe, dIm)
  auto make_d = [&](int bg, const Raw& w, float (&dre)[4], float (&dim)[4]) {
    const float rv[4] = {w.re.x, w.re.y, w.re.z, w.re.w}, iv[4] = {w.im.x, w.im.y, w.im.z, w.im.w};
    const float ymv[4] = {w.ym.x, w.ym.y, w.ym.z, w.ym.w}, ylv[4] = {w.yl.x, w.yl.y, w.yl.z, w.yl.w};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      dre[s] = dim[s] = 0.f;
      if (!valid || bg * 16 + fk + s >= SF_NB) continue;
      const float p = rv[s] * rv[s] + iv[s] * iv[s];
      if (!(p > SF_EPS)) continue;  // the clamp: no gradient
      const float xm = sqrtf(p);
      const float df = logf(xm) - ylv[s];
      const float sg = df > 0.f ? 1.0f : (df < 0.f ? -1.0f : 0.f);
      const float d = (xm - ymv[s]) * c1 + (sg * c2) / xm;
      const float q = d / xm;
      dre[s] = q * rv[s];
      dim[s] = q * iv[s];
    }
  };
  auto load_b = [&](int bg, float4 (&bc)[SF_BWT], float4 (&bs)[SF_BWT]) {
#pragma unroll
    for (int j = 0; j < SF_BWT; ++j) {
      const size_t o = ((size_t)bg * SF_N + (nt0 + j) * 16 + fr) * 16 + fk;
      bc[j] = *(const float4*)(basisT + o);
      bs[j] = *(const float4*)(basisT + (size_t)SF_NBT * SF_N * 16 + o);
    }
  };
  auto step = [&](const float (&dre)[4], const float (&dim)[4], const float4 (&bc)[SF_BWT],
                  const float4 (&bs)[SF_BWT], f32x4 (&a)[SF_BWT]) {
#pragma unroll
    for (int j = 0; j < SF_BWT; ++j) {
      a[j] = sf_mfma(bc[j].x, dre[0], a[j]);
      a[j] = sf_mfma(bc[j].y, dre[1], a[j]);
      a[j] = sf_mfma(bc[j].z, dre[2], a[j]);
      a[j] = sf_mfma(bc[j].w, dre[3], a[j]);
      a[j] = sf_mfma(bs[j].x, dim[0], a[j]);
      a[j] = sf_mfma(bs[j].y, dim[1], a[j]);
      a[j] = sf_mfma(bs[j].z, dim[2], a[j]);
      a[j] = sf_mfma(bs[j].w, dim[3], a[j]);
    }
  };

  Raw raw = {};
  float4 bcA[SF_BWT], bsA[SF_BWT], bcB[SF_BWT], bsB[SF_BWT];
  float drA[4], diA[4], drB[4], diB[4];
  load_raw(0, raw);
  load_b(0, bcA, bsA);
  make_d(0, raw, drA, diA);
  for (int bg = 0; bg < SF_NBT; bg += 2) {
    const bool odd = bg + 1 < SF_NBT, next = bg + 2 < SF_NBT;
    if (odd) {
      load_raw(bg + 1, raw);
      load_b(bg + 1, bcB, bsB);
    }
    step(drA, diA, bcA, bsA, acc[0]);
    if (odd) make_d(bg + 1, raw, drB, diB);
    if (next) {
      load_raw(bg + 2, raw);
      load_b(bg + 2, bcA, bsA);
    }
    if (odd) step(drB, diB, bcB, bsB, acc[1]);
    if (next) make_d(bg + 2, raw, drA, diA);
  }
  // lane: frame t, samples (nt0 + j) 16 + fk + r of the frame
  if (valid) {
#pragma unroll
    for (int j = 0; j < SF_BWT; ++j) {
      const f32x4 v = acc[0][j] + acc[1][j];
      *(float4*)(dF + (size_t)t * SF_N + (nt0 + j) * 16 + fk) = float4{v[0], v[1], v[2], v[3]};
    }
  }
}

// contributions of padded index j: the frames 256 t <= j < 256 t + 1024, t < T, ascending
__device__ __forceinline__ float gather_j(const float* __restrict__ dF, int64_t j, int T) {
  const int64_t tlo = j < SF_N ? 0 : (j - SF_N) / SF_HOP + 1;
  int64_t thi = j / SF_HOP;
  if (thi > T - 1) thi = T - 1;
  float s = 0.f;
  for (int64_t t = tlo; t <= thi; ++t) s += dF[t * SF_N + (j - t * SF_HOP)];
  return s;
}
// dL_stft/dx_i: sample i itself (padded index i + 512), its image in the left reflection
// (512 - i, i in 1..512) and in the right one (2 (n - 1) - i + 512, i in n - 513..n - 2), in that order
__device__ __forceinline__ float gather_sample(const float* __restrict__ dF, int i, int n, int T) {
  float s = gather_j(dF, (int64_t)i + SF_N / 2, T);
  if (i >= 1 && i <= SF_N / 2) s += gather_j(dF, SF_N / 2 - i, T);
  if (i <= n - 2 && i >= n - SF_N / 2 - 1) s += gather_j(dF, 2 * (int64_t)(n - 1) - i + SF_N / 2, T);
  return s;
}

__global__ void stft_gather_kernel(const float* __restrict__ dF, int n, int T, float* __restrict__ g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) g[i] = gather_sample(dF, i, n, T);
}

// sums of x and y per 256 samples
__global__ void snr_sums1_kernel(const float* __restrict__ x, const float* __restrict__ y, int n,
                                 float* __restrict__ part, int npart) {
  __shared__ float scratch[4];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const float sx = block_sum(i < n ? x[i] : 0.f, scratch);
  const float sy = block_sum(i < n ? y[i] : 0.f, scratch);
  if (threadIdx.x == 0) {
    part[(size_t)PT_SX * npart + blockIdx.x] = sx;
    part[(size_t)PT_SYM * npart + blockIdx.x] = sy;
  }
}

// block_sum (siren_common.h) in fp64: fixed order, valid in every thread; scratch: blockDim.x / 64 doubles
__device__ __forceinline__ double block_sum_d(double v, double* scratch) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < nw; ++i) s += scratch[i];
  return s;
}

// the means (every block sums the partials in the same order), then sums of yc^2 and (xc - yc)^2,
// formed and summed in fp64 and stored as hi + lo floats
__global__ void snr_sums2_kernel(const float* __restrict__ x, const float* __restrict__ y, int n,
                                 float* __restrict__ part, int npart, int nblk, float* __restrict__ scal) {
  __shared__ float scratch[4];
  float ax = 0.f, ay = 0.f;
  for (int k = threadIdx.x; k < nblk; k += blockDim.x) {
    ax += part[(size_t)PT_SX * npart + k];
    ay += part[(size_t)PT_SYM * npart + k];
  }
  __shared__ double scratch_d[4];
  const float mx = block_sum(ax, scratch) / (float)n, my = block_sum(ay, scratch) / (float)n;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double yc = 0.0, r = 0.0;
  if (i < n) {
    yc = (double)y[i] - (double)my;
    r = ((double)x[i] - (double)mx) - yc;
  }
  const double syc = block_sum_d(yc * yc, scratch_d);
  const double sr = block_sum_d(r * r, scratch_d);
  if (threadIdx.x == 0) {
    const float syc_hi = (float)syc, sr_hi = (float)sr;
    part[(size_t)PT_SYC * npart + blockIdx.x] = syc_hi;
    part[(size_t)PT_SR * npart + blockIdx.x] = sr_hi;
    part[(size_t)PT_SYC_LO * npart + blockIdx.x] = (float)(syc - (double)syc_hi);
    part[(size_t)PT_SR_LO * npart + blockIdx.x] = (float)(sr - (double)sr_hi);
    if (blockIdx.x == 0) {
      scal[SC_MX] = mx;
      scal[SC_MY] = my;
    }
  }
}

// the finished scalars (one block, fp64 sums of the fp32 partials in a fixed order):
//   nstft > 0: S1, sum|dlog| -> L_stft, c1 = 1 / (sqrt S1 sqrt Sy), c2 = 1 / (T 513)
//   loss_mode 2: L_snr and the gradient factor; 0 / 1: the mean of sse_part's sum (MSE / L1); -1: none
//   loss = (1 - alpha) point + alpha L_stft (loss_mode -1: L_stft), fp32, also to loss_out[0]
__global__ __launch_bounds__(256) void loss_finish_kernel(float* __restrict__ scal, const float* __restrict__ part,
                                                          int npart, int nstft, int nsnr,
                                                          const float* __restrict__ sse_part, int nsum,
                                                          int loss_mode, double alpha, double n_total, int T,
                                                          float* __restrict__ loss_out) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  auto total = [&](const float* p, int cnt) {  // valid in thread 0
    double a = 0.0;
    for (int k = tid; k < cnt; k += 256) a += (double)p[k];
    __syncthreads();
    sh[tid] = a;
    __syncthreads();
    double s = 0.0;
    if (tid == 0)
      for (int k = 0; k < 256; ++k) s += sh[k];
    return s;
  };
  double lstft = 0.0, lpoint = 0.0;
  if (nstft > 0) {
    const double S1 = total(part + (size_t)PT_S1 * npart, nstft);
    const double SL = total(part + (size_t)PT_SL * npart, nstft);
    if (tid == 0) {
      const double Sy = (double)scal[SC_SY];
      const double r1 = sqrt(S1), ry = sqrt(Sy), cnt = (double)T * SF_NB;
      lstft = r1 / ry + SL / cnt;
      scal[SC_S1] = (float)S1;
      scal[SC_SL] = (float)SL;
      scal[SC_LSTFT] = (float)lstft;
      scal[SC_C1] = (S1 > 0.0 && Sy > 0.0) ? (float)(1.0 / (r1 * ry)) : 0.f;
      scal[SC_C2] = (float)(1.0 / cnt);
    }
  }
  if (loss_mode == 2) {
    const double Syc = total(part + (size_t)PT_SYC * npart, nsnr) + total(part + (size_t)PT_SYC_LO * npart, nsnr);
    const double Sr = total(part + (size_t)PT_SR * npart, nsnr) + total(part + (size_t)PT_SR_LO * npart, nsnr);
    if (tid == 0) {
      const double eps = 1e-8, q = Syc / (Sr + eps);
      lpoint = -10.0 * log10(q + eps);
      scal[SC_SYC] = (float)Syc;
      scal[SC_SR] = (float)Sr;
      scal[SC_LSNR] = (float)lpoint;
      scal[SC_FSNR] = (float)((10.0 / log(10.0)) * (q / (q + eps)) * (2.0 / (Sr + eps)));
    }
  } else if (loss_mode >= 0) {
    const double se = total(sse_part, nsum);
    if (tid == 0) lpoint = se / n_total;
  }
  if (tid == 0) {
    const double loss = loss_mode < 0 ? lstft : (1.0 - alpha) * lpoint + alpha * lstft;
    scal[SC_LPOINT] = (float)lpoint;
    scal[SC_LOSS] = (float)loss;
    if (loss_out) loss_out[0] = (float)loss;
  }
}

// g = (1 - alpha) g_point + alpha g_stft over the valid rows, 0 on pad rows
__global__ void loss_mix_kernel(const float* __restrict__ out, const float* __restrict__ y, int n, int rows,
                                const float* __restrict__ dF, int T, const float* __restrict__ scal, int loss_mode,
                                float wp, float ws, float gfac, float* __restrict__ g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  float v = 0.f;
  if (i < n) {
    float gp;
    if (loss_mode == 2) {
      gp = scal[SC_FSNR] * ((out[i] - scal[SC_MX]) - (y[i] - scal[SC_MY]));
    } else {
      const float err = out[i] - y[i];
      gp = loss_mode == 1 ? (err > 0.f ? 1.0f : (err < 0.f ? -1.0f : 0.f)) * gfac : err * gfac;
    }
    v = wp * gp;
    if (ws != 0.f) v += ws * gather_sample(dF, i, n, T);
  }
  g[i] = v;
}

inline size_t up4(size_t v) { return (v + 3) / 4 * 4; }

}  // namespace

int64_t stft_frames(int64_t n) { return n > SF_N / 2 ? 1 + n / SF_HOP : 0; }

int64_t stft_basis_floats() { return (int64_t)(2 * SF_TAB); }

void stft_basis_fill(float* host) {
  const double two_pi = 6.283185307179586476925286766559;
  float* fwd = host;
  float* bwd = host + SF_TAB;
  for (size_t i = 0; i < 2 * SF_TAB; ++i) host[i] = 0.f;
  for (int k = 0; k < SF_N; ++k) {
    const double w = 0.5 - 0.5 * cos(two_pi * k / SF_N);  // periodic Hann
    for (int b = 0; b < SF_NB; ++b) {
      const double th = two_pi * (double)((k * b) % SF_N) / SF_N;  // the angle reduced exactly
      const float v[2] = {(float)(w * cos(th)), (float)(-w * sin(th))};
      for (int c = 0; c < 2; ++c) {
        fwd[(((size_t)c * SF_KT + k / 16) * SF_NBP + b) * 16 + k % 16] = v[c];
        bwd[(((size_t)c * SF_NBT + b / 16) * SF_N + k) * 16 + b % 16] = v[c];
      }
    }
  }
}

static int stft_npart(int n, int rows) {
  const int a = (int)((stft_frames(n) + SF_FT - 1) / SF_FT) * SF_FGY, b = (rows + 255) / 256;
  return (int)up4(a > b ? a : b);
}

int64_t stft_ws_floats(int n, int rows) {
  const size_t T = (size_t)stft_frames(n);
  return (int64_t)(4 * T * SF_NBP + T * SF_N + PT_ROWS * (size_t)stft_npart(n, rows) + 32 + up4(rows));
}

StftWs stft_ws_map(float* ws, int n, int rows) {
  StftWs w;
  const size_t T = (size_t)stft_frames(n);
  w.T = (int)T;
  w.npart = stft_npart(n, rows);
  w.re = ws;
  w.im = w.re + T * SF_NBP;
  w.ymag = w.im + T * SF_NBP;
  w.ylog = w.ymag + T * SF_NBP;
  w.dF = w.ylog + T * SF_NBP;
  w.part = w.dF + T * SF_N;
  w.scal = w.part + PT_ROWS * (size_t)w.npart;
  w.gchain = w.scal + 32;
  return w;
}

hipError_t stft_forward(const float* x, int n, const float* basis, const StftWs& w, bool target, hipStream_t s) {
  if (w.T < 1) return hipErrorInvalidValue;
  const dim3 grid((w.T + SF_FT - 1) / SF_FT, SF_FGY);
  if (target) {
    hipLaunchKernelGGL(stft_fwd_kernel<true>, grid, dim3(256), 0, s, x, n, w.T, basis, w.ymag, w.ylog, nullptr, nullptr,
                       w.part, w.npart);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return sum_to(w.part + (size_t)PT_S1 * w.npart, (int)(grid.x * grid.y), w.scal + SC_SY, 0, s);
  }
  hipLaunchKernelGGL(stft_fwd_kernel<false>, grid, dim3(256), 0, s, x, n, w.T, basis, w.re, w.im, w.ymag, w.ylog,
                     w.part, w.npart);
  return hipGetLastError();
}

hipError_t snr_sums(const float* x, const float* y, int n, const StftWs& w, hipStream_t s) {
  const int nblk = (n + 255) / 256;
  hipLaunchKernelGGL(snr_sums1_kernel, dim3(nblk), dim3(256), 0, s, x, y, n, w.part, w.npart);
  hipLaunchKernelGGL(snr_sums2_kernel, dim3(nblk), dim3(256), 0, s, x, y, n, w.part, w.npart, nblk, w.scal);
  return hipGetLastError();
}

hipError_t loss_finish(const StftWs& w, int n, const float* sse_part, int nsum, int loss_mode, double alpha,
                       double n_total, bool stft, float* loss_out, hipStream_t s) {
  const int nstft = stft ? (w.T + SF_FT - 1) / SF_FT * SF_FGY : 0;
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, s, w.scal, w.part, w.npart, nstft, (n + 255) / 256,
                     sse_part, nsum, loss_mode, alpha, n_total, w.T, loss_out);
  return hipGetLastError();
}

hipError_t stft_backward(const float* basis, const StftWs& w, hipStream_t s) {
  if (w.T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(stft_bwd_kernel, dim3((w.T + SF_FT - 1) / SF_FT, SF_BGY), dim3(256), 0, s, w.T, basis + SF_TAB,
                     w.re, w.im, w.ymag, w.ylog, w.scal, w.dF);
  return hipGetLastError();
}

hipError_t stft_gather(int n, const StftWs& w, float* g_stft, hipStream_t s) {
  hipLaunchKernelGGL(stft_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, w.dF, n, w.T, g_stft);
  return hipGetLastError();
}

hipError_t loss_mix(const float* out, const float* y, int n, int rows, const StftWs& w, int loss_mode, double alpha,
                    float gfac, float* g, hipStream_t s) {
  hipLaunchKernelGGL(loss_mix_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, out, y, n, rows, w.dF, w.T, w.scal,
                     loss_mode, (float)(1.0 - alpha), (float)alpha, gfac, g);
  return hipGetLastError();
}

}  // namespace siren
