// Multi-resolution STFT loss (run.py:127, :160: auraloss.freq.MultiResolutionSTFTLoss(), restated
// from its published 0.4.0 defaults; perceptual_weighting=False) for the model output x and the
// target y, both one sequence of n > 1024 samples:
//
//   r   n_fft   hop   win    left zero-pad   bins   frames T_r
//   0   1024    120    600        212         513   1 + n / 120
//   1   2048    240   1200        424        1025   1 + n / 240
//   2    512     50    240        136         257   1 + n / 50
//   X_r = stft(x, n_fft, hop, periodic Hann(win) centred in the n_fft frame, center, reflect)
//   x_mag = sqrt(max(re^2 + im^2, 1e-8))
//   L_r = ||y_mag - x_mag||_F / ||y_mag||_F + mean |log x_mag - log y_mag|
//   L_mrstft = (L_0 + L_1 + L_2) / 3,  loss = (1 - alpha) {MSE | L1 | SNR} + alpha L_mrstft
//
// As in stft.hip each transform is an exact-fp32 GEMM on v_mfma_f32_16x16x4_f32 against windowed
// cos / -sin tables (fp64 on the host, rounded once; no fp16 operands, stft.hip:11-12).  What differs:
//
// K runs over the window's support only.  Taps outside [pad, pad + win) carry a zero window, so the
// table holds the rows k' = tap - pad < KWP = win rounded up to the 16-k group (608 / 1200 / 240; the
// rows past win are zero) and frame t reads the padded samples t hop + pad + k'.
//   fwd[c][k' / 16][bin][k' % 16]    bwd[c][bin / 16][k'][bin % 16]    (c: 0 = w cos, 1 = -w sin;
//   bin < NBP = 528 / 1040 / 272, zero past the last bin), per resolution, one after the other.
//
// mr_fwd_kernel<R>: a block owns 16 frames and 4 x WT bin tiles of 16 (WT per wave).  The frames
// are read from the signal staged once in LDS (reflection folded in the staging index), never as a
// [T][n_fft] matrix.  A lane (fr = l & 15, kq = l >> 4) reads the float4 at tap 16 kt + 4 kq of frame fr;
// one ds_read_b128 is served in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and
// the same + 32: a group holds all 16 frames, frames 0-3 and 12-15 at one kq and frames 4-11 at the
// next.  A read is conflict-free when the 16 float4 slots (address / 4 mod 16) of a group differ.
//   r = 0 (hop 120 = 30 slots = -2 mod 16): sig[2408], padded sample q at q.  Slot -2 fr + kq: frames
//     fr and fr + 8 share -2 fr, and exactly one of the two sits at the odd kq -- all 16 differ.
//     Every address is a multiple of 4 floats (120, 16, 4).
//   r = 1 (hop 240 = 60 slots = -4 mod 16, 4 distinct values: 4-way): sig[4960], sample q at
//     q + 8 (q / 240): the frame stride becomes 248 floats = 62 slots = -2 mod 16, the case above.
//     q / 240 = fr + kt / 15 (240 = 15 groups of 16), the same for a whole 16-k group, so a float4
//     stays contiguous and 16-B aligned.  Its table (10 MB per layout) does not fit an XCD's 4 MB L2;
//     keeping each table piece for 32 frames per block (half the table traffic, 35 KB of LDS) measured
//     2 % slower than 16 frames per block, so every resolution takes 16.
//   r = 2 (hop 50 = 200 B: odd frames are only 8-B aligned, a ds_read_b128 there is replayed): the 16
//     frames get a pitch of their own, sig[16][248] (pitch 62 slots = -2 mod 16, as above), 15.9 KB;
//     the 240 taps of a frame are staged from global memory (L1 / L2 hits: frames overlap 4.8-fold).
// K is accumulated in two interleaved chains (even / odd 16-k groups), summed at the end: fma chains
// of at most 304 / 608 / 128 terms.
//
// mr_bwd_kernel<R>: dF[T][KWP] = [dRe | dIm] x bwd table; the B operand is formed from re / im, the
// target's magnitudes and the finished scalars as it is loaded (stft.hip:32-37, with c2 = 1 / (T_r bins)).
// The gather sums, per sample, the <= 5 frames that cover it (win / hop <= 5) and the same for its
// reflected images, ascending, then adds the resolutions in the order 0, 1, 2, each times 1/3 -- no
// float atomics anywhere, two runs are bit-identical.  The scalars are finished in fp64 on the device.
#include <math.h>
#include "siren_common.h"
#include "siren_kernels.h"

namespace siren {

namespace {

constexpr float MR_EPS = 1e-8f;
constexpr float MR_THIRD = 1.0f / 3.0f;

template <int NFFT_, int HOP_, int WIN_, int WT_, int BWT_, int PITCH_, int SKEW_>
struct MrTraits {
  static constexpr int NFFT = NFFT_, HOP = HOP_, WIN = WIN_, PADL = (NFFT_ - WIN_) / 2;
  static constexpr int NB = NFFT_ / 2 + 1, NBP = (NB + 15) / 16 * 16, NBT = NBP / 16;
  static constexpr int KT = (WIN_ + 15) / 16, KWP = KT * 16;      // 16-k groups / table rows
  static constexpr int FT = 16;                                   // frames per block
  static constexpr int WT = WT_, FGY = (NBT + 4 * WT_ - 1) / (4 * WT_);   // bin tiles per wave, grid.y
  static constexpr int BWT = BWT_, BGY = (KT + 4 * BWT_ - 1) / (4 * BWT_);  // backward: tap tiles per wave
  static constexpr int PITCH = PITCH_, SKEW = SKEW_;
  static constexpr int SEG = (FT - 1) * HOP_ + KWP;               // padded samples a block's frames span
  static constexpr int LDS = PITCH_ ? FT * PITCH_ : SEG + SKEW_ * ((SEG + HOP_ - 1) / HOP_);
  static constexpr size_t TAB = (size_t)2 * KWP * NBP;            // floats of one table layout
  static_assert(SKEW_ == 0 || HOP_ % 16 == 0, "the skew is constant over a 16-k group");
  static_assert(PITCH_ % 4 == 0 && SKEW_ % 4 == 0 && (PITCH_ || HOP_ % 4 == 0), "16-B aligned float4 reads");
  static_assert(PITCH_ == 0 || PITCH_ >= KWP, "a frame's taps fit its pitch");
  // LDS index of tap 16 kt + fk (fk = 0, 4, 8, 12; + 0..3) of the block's frame f
  __device__ static __forceinline__ int at(int f, int kt, int fk) {
    if constexpr (PITCH_ != 0) return PITCH_ * f + 16 * kt + fk;
    else if constexpr (SKEW_ != 0) return HOP_ * f + 16 * kt + fk + SKEW_ * (f + kt / (HOP_ / 16));
    else return HOP_ * f + 16 * kt + fk;
  }
};
//                  n_fft  hop   win  WT BWT pitch skew
using MrR0 = MrTraits<1024, 120, 600, 3, 5, 0, 0>;
using MrR1 = MrTraits<2048, 240, 1200, 3, 4, 0, 8>;
using MrR2 = MrTraits<512, 50, 240, 5, 4, 248, 0>;

__device__ __forceinline__ f32x4 mr_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// sample at padded index j of the centred, reflect-padded signal (0 past the padded end: frames >= T);
// n > 1024 >= n_fft / 2, so one reflection lands inside the signal
template <int NFFT>
__device__ __forceinline__ float mr_sample(const float* __restrict__ x, int n, int64_t j) {
  int64_t i = j - NFFT / 2;
  if (i < 0) {
    i = -i;
  } else if (i >= n) {
    i = 2 * (int64_t)(n - 1) - i;
    if (i < 0) return 0.f;
  }
  return x[i];
}

template <class R, bool TARGET>
__global__ __launch_bounds__(256) void mr_fwd_kernel(const float* __restrict__ x, int n, int T,
                                                     const float* __restrict__ basis, float* __restrict__ o0,
                                                     float* __restrict__ o1, const float* __restrict__ ymag,
                                                     const float* __restrict__ ylog, float* __restrict__ part,
                                                     int npart) {
  constexpr int WT = R::WT;
  __shared__ __attribute__((aligned(16))) float sig[R::LDS];
  __shared__ float scratch[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t0 = blockIdx.x * R::FT;
  const int64_t j0 = (int64_t)t0 * R::HOP + R::PADL;
  if constexpr (R::PITCH != 0) {
    for (int e = tid; e < R::FT * R::KWP; e += 256) {
      const int f = e / R::KWP, u = e - f * R::KWP;
      sig[R::PITCH * f + u] = mr_sample<R::NFFT>(x, n, j0 + f * R::HOP + u);
    }
  } else {
    for (int q = tid; q < R::SEG; q += 256) sig[q + R::SKEW * (q / R::HOP)] = mr_sample<R::NFFT>(x, n, j0 + q);
  }
  __syncthreads();

  const int fr = lane & 15, fk = 4 * (lane >> 4);
  const int bt0 = (blockIdx.y * 4 + wave) * WT;
  f32x4 ac[2][WT], as[2][WT];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < WT; ++j) ac[h][j] = as[h][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto load_b = [&](int kt, float4 (&bc)[WT], float4 (&bs)[WT]) {
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      // a tile past the last one re-reads the last: its results are not stored, and without a
      // branch here the pieces stay in registers
      const int bt = bt0 + j < R::NBT ? bt0 + j : R::NBT - 1;
      const size_t o = ((size_t)kt * R::NBP + bt * 16 + fr) * 16 + fk;
      bc[j] = *(const float4*)(basis + o);
      bs[j] = *(const float4*)(basis + (size_t)R::KWP * R::NBP + o);
    }
  };
  auto step = [&](int kt, const float4 (&bc)[WT], const float4 (&bs)[WT], f32x4 (&c)[WT], f32x4 (&s)[WT]) {
    const float4 a = *(const float4*)&sig[R::at(fr, kt, fk)];
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      c[j] = mr_mfma(bc[j].x, a.x, c[j]);
      s[j] = mr_mfma(bs[j].x, a.x, s[j]);
      c[j] = mr_mfma(bc[j].y, a.y, c[j]);
      s[j] = mr_mfma(bs[j].y, a.y, s[j]);
      c[j] = mr_mfma(bc[j].z, a.z, c[j]);
      s[j] = mr_mfma(bs[j].z, a.z, s[j]);
      c[j] = mr_mfma(bc[j].w, a.w, c[j]);
      s[j] = mr_mfma(bs[j].w, a.w, s[j]);
    }
  };
  // the next 16-k group's table pieces travel under this group's MFMAs
  float4 bcA[WT], bsA[WT], bcB[WT], bsB[WT];
  load_b(0, bcA, bsA);
  for (int kt = 0; kt < R::KT; kt += 2) {
    const bool odd = kt + 1 < R::KT;
    if (odd) load_b(kt + 1, bcB, bsB);
    step(kt, bcA, bsA, ac[0], as[0]);
    if (kt + 2 < R::KT) load_b(kt + 2, bcA, bsA);
    if (odd) step(kt + 1, bcB, bsB, ac[1], as[1]);
  }

  // lane: frame t0 + fr, bins (bt0 + j) 16 + fk + r
  float s1 = 0.f, sl = 0.f;
  const int t = t0 + fr;
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    if (bt0 + j >= R::NBT || t >= T) continue;
    const f32x4 re = ac[0][j] + ac[1][j], im = as[0][j] + as[1][j];
    const size_t o = (size_t)t * R::NBP + (bt0 + j) * 16 + fk;
    float mag[4], lg[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mag[r] = sqrtf(fmaxf(re[r] * re[r] + im[r] * im[r], MR_EPS));
      lg[r] = logf(mag[r]);
    }
    if constexpr (TARGET) {
      *(float4*)(o0 + o) = float4{mag[0], mag[1], mag[2], mag[3]};
      *(float4*)(o1 + o) = float4{lg[0], lg[1], lg[2], lg[3]};
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if ((bt0 + j) * 16 + fk + r < R::NB) s1 += mag[r] * mag[r];
    } else {
      *(float4*)(o0 + o) = float4{re[0], re[1], re[2], re[3]};
      *(float4*)(o1 + o) = float4{im[0], im[1], im[2], im[3]};
      const float4 ym = *(const float4*)(ymag + o), yl = *(const float4*)(ylog + o);
      const float ymv[4] = {ym.x, ym.y, ym.z, ym.w}, ylv[4] = {yl.x, yl.y, yl.z, yl.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if ((bt0 + j) * 16 + fk + r < R::NB) {
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
    part[blk] = s1;
    part[(size_t)npart + blk] = sl;
  }
}

template <class R>
__global__ __launch_bounds__(256) void mr_bwd_kernel(int T, const float* __restrict__ basisT,
                                                     const float* __restrict__ re, const float* __restrict__ im,
                                                     const float* __restrict__ ymag, const float* __restrict__ ylog,
                                                     const float* __restrict__ scal, float* __restrict__ dF) {
  constexpr int BWT = R::BWT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fk = 4 * (lane >> 4);
  const int t = blockIdx.x * R::FT + fr;
  const bool valid = t < T;
  const int nt0 = (blockIdx.y * 4 + wave) * BWT;
  const float c1 = scal[MR_C1], c2 = scal[MR_C2];
  f32x4 acc[2][BWT];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < BWT; ++j) acc[h][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  struct Raw { float4 re, im, ym, yl; };
  auto load_raw = [&](int bg, Raw& w) {
    if (valid) {
      const size_t o = (size_t)t * R::NBP + bg * 16 + fk;
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
      if (!valid || bg * 16 + fk + s >= R::NB) continue;
      const float p = rv[s] * rv[s] + iv[s] * iv[s];
      if (!(p > MR_EPS)) continue;  // the clamp: no gradient
      const float xm = sqrtf(p);
      const float df = logf(xm) - ylv[s];
      const float sg = df > 0.f ? 1.0f : (df < 0.f ? -1.0f : 0.f);
      const float d = (xm - ymv[s]) * c1 + (sg * c2) / xm;
      const float q = d / xm;
      dre[s] = q * rv[s];
      dim[s] = q * iv[s];
    }
  };
  auto load_b = [&](int bg, float4 (&bc)[BWT], float4 (&bs)[BWT]) {
#pragma unroll
    for (int j = 0; j < BWT; ++j) {
      const int nt = nt0 + j < R::KT ? nt0 + j : R::KT - 1;   // a tile past the last: not stored
      const size_t o = ((size_t)bg * R::KWP + nt * 16 + fr) * 16 + fk;
      bc[j] = *(const float4*)(basisT + o);
      bs[j] = *(const float4*)(basisT + (size_t)R::NBT * R::KWP * 16 + o);
    }
  };
  auto step = [&](const float (&dre)[4], const float (&dim)[4], const float4 (&bc)[BWT], const float4 (&bs)[BWT],
                  f32x4 (&a)[BWT]) {
#pragma unroll
    for (int j = 0; j < BWT; ++j) {
      a[j] = mr_mfma(bc[j].x, dre[0], a[j]);
      a[j] = mr_mfma(bc[j].y, dre[1], a[j]);
      a[j] = mr_mfma(bc[j].z, dre[2], a[j]);
      a[j] = mr_mfma(bc[j].w, dre[3], a[j]);
      a[j] = mr_mfma(bs[j].x, dim[0], a[j]);
      a[j] = mr_mfma(bs[j].y, dim[1], a[j]);
      a[j] = mr_mfma(bs[j].z, dim[2], a[j]);
      a[j] = mr_mfma(bs[j].w, dim[3], a[j]);
    }
  };

  Raw raw = {};
  float4 bcA[BWT], bsA[BWT], bcB[BWT], bsB[BWT];
  float drA[4], diA[4], drB[4], diB[4];
  load_raw(0, raw);
  load_b(0, bcA, bsA);
  make_d(0, raw, drA, diA);
  for (int bg = 0; bg < R::NBT; bg += 2) {
    const bool odd = bg + 1 < R::NBT, next = bg + 2 < R::NBT;
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
  // lane: frame t, taps (nt0 + j) 16 + fk + r of the window's support
  if (valid) {
#pragma unroll
    for (int j = 0; j < BWT; ++j) {
      if (nt0 + j >= R::KT) continue;
      const f32x4 v = acc[0][j] + acc[1][j];
      *(float4*)(dF + (size_t)t * R::KWP + (nt0 + j) * 16 + fk) = float4{v[0], v[1], v[2], v[3]};
    }
  }
}

// contributions of padded index j: the frames t hop + pad <= j < t hop + pad + win, t < T, ascending
template <class R>
__device__ __forceinline__ float mr_gather_j(const float* __restrict__ dF, int64_t j, int T) {
  const int64_t a = j - R::PADL;   // tap 0 of frame t sits at a = t hop
  if (a < 0) return 0.f;
  const int64_t tlo = a < R::WIN ? 0 : (a - R::WIN) / R::HOP + 1;
  int64_t thi = a / R::HOP;
  if (thi > T - 1) thi = T - 1;
  float s = 0.f;
  for (int64_t t = tlo; t <= thi; ++t) s += dF[t * R::KWP + (a - t * R::HOP)];
  return s;
}
// dL_r/dx_i: sample i itself (padded index i + n_fft / 2), its image in the left reflection
// (n_fft / 2 - i, i in 1..n_fft / 2) and in the right one (2 (n - 1) - i + n_fft / 2, i in
// n - 1 - n_fft / 2..n - 2), in that order
template <class R>
__device__ __forceinline__ float mr_gather_sample(const float* __restrict__ dF, int i, int n, int T) {
  constexpr int H = R::NFFT / 2;
  float s = mr_gather_j<R>(dF, (int64_t)i + H, T);
  if (i >= 1 && i <= H) s += mr_gather_j<R>(dF, H - i, T);
  if (i <= n - 2 && i >= n - H - 1) s += mr_gather_j<R>(dF, 2 * (int64_t)(n - 1) - i + H, T);
  return s;
}

struct MrGather {
  const float* dF[kMrRes];
  int T[kMrRes];
};
// dL_mrstft/dx_i: the three resolutions in the order 0, 1, 2, each times 1/3
__device__ __forceinline__ float mr_gather3(const MrGather& ga, int i, int n) {
  float s = MR_THIRD * mr_gather_sample<MrR0>(ga.dF[0], i, n, ga.T[0]);
  s += MR_THIRD * mr_gather_sample<MrR1>(ga.dF[1], i, n, ga.T[1]);
  s += MR_THIRD * mr_gather_sample<MrR2>(ga.dF[2], i, n, ga.T[2]);
  return s;
}

__global__ void mr_gather_kernel(MrGather ga, int n, float* __restrict__ g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) g[i] = mr_gather3(ga, i, n);
}

// g = (1 - alpha) g_point + alpha g_mrstft over the valid rows, 0 on pad rows (stft.hip loss_mix_kernel
// with the three-resolution gather; pscal: the point loss's scalars)
__global__ void mr_mix_kernel(const float* __restrict__ out, const float* __restrict__ y, int n, int rows,
                              MrGather ga, const float* __restrict__ pscal, int loss_mode, float wp, float ws,
                              float gfac, float* __restrict__ g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  float v = 0.f;
  if (i < n) {
    float gp;
    if (loss_mode == 2) {
      gp = pscal[SC_FSNR] * ((out[i] - pscal[SC_MX]) - (y[i] - pscal[SC_MY]));
    } else {
      const float err = out[i] - y[i];
      gp = loss_mode == 1 ? (err > 0.f ? 1.0f : (err < 0.f ? -1.0f : 0.f)) * gfac : err * gfac;
    }
    v = wp * gp;
    if (ws != 0.f) v += ws * mr_gather3(ga, i, n);
  }
  g[i] = v;
}

struct MrFinish {
  const float* part[kMrRes];
  int npart[kMrRes], nblk[kMrRes], T[kMrRes], NB[kMrRes];
};
// the finished scalars (one block, fp64 sums of the fp32 partials in a fixed order), per resolution
//   S1, sum|dlog| -> L_r, c1 = 1 / (sqrt S1 sqrt Sy), c2 = 1 / (T_r bins)
// then L_mrstft = (L_0 + L_1 + L_2) / 3 and loss = (1 - alpha) point + alpha L_mrstft (loss_mode -1:
// L_mrstft), the point loss from loss_finish's scalars.  nres 0: no spectral term (loss = point).
// loss_out[0] <- loss; terms: loss_out[1..3] <- L_0, L_1, L_2
__global__ __launch_bounds__(256) void mr_finish_kernel(MrFinish f, int nres, float* __restrict__ scal,
                                                        const float* __restrict__ pscal, int loss_mode, double alpha,
                                                        float* __restrict__ loss_out, int terms) {
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
  double lsum = 0.0;
  for (int r = 0; r < nres; ++r) {
    const double S1 = total(f.part[r], f.nblk[r]);
    const double SL = total(f.part[r] + f.npart[r], f.nblk[r]);
    if (tid == 0) {
      float* sc = scal + MR_SLOTS * r;
      const double Sy = (double)sc[MR_SY];
      const double r1 = sqrt(S1), ry = sqrt(Sy), cnt = (double)f.T[r] * f.NB[r];
      const double l = r1 / ry + SL / cnt;
      sc[MR_S1] = (float)S1;
      sc[MR_SL] = (float)SL;
      sc[MR_L] = (float)l;
      sc[MR_C1] = (S1 > 0.0 && Sy > 0.0) ? (float)(1.0 / (r1 * ry)) : 0.f;
      sc[MR_C2] = (float)(1.0 / cnt);
      if (terms) loss_out[1 + r] = (float)l;
      lsum += l;
    }
  }
  if (tid == 0) {
    const double lmr = nres > 0 ? lsum / 3.0 : 0.0;
    const double lpoint = loss_mode < 0 ? 0.0 : (double)pscal[SC_LPOINT];
    const double loss = loss_mode < 0 ? lmr : (1.0 - alpha) * lpoint + alpha * lmr;
    scal[MR_SLOTS * kMrRes + MR_MEAN] = (float)lmr;
    scal[MR_SLOTS * kMrRes + MR_POINT] = (float)lpoint;
    scal[MR_SLOTS * kMrRes + MR_LOSS] = (float)loss;
    if (loss_out) loss_out[0] = (float)loss;
  }
}

inline size_t up4(size_t v) { return (v + 3) / 4 * 4; }

template <class R>
int64_t frames_of(int64_t n) { return 1 + n / R::HOP; }

template <class R>
int npart_of(int64_t T) { return (int)up4((size_t)((T + R::FT - 1) / R::FT) * R::FGY); }

template <class R>
void fill_tables(float* fwd) {
  const double two_pi = 6.283185307179586476925286766559;
  float* bwd = fwd + R::TAB;
  for (size_t i = 0; i < 2 * R::TAB; ++i) fwd[i] = 0.f;
  for (int k = 0; k < R::WIN; ++k) {
    const double w = 0.5 - 0.5 * cos(two_pi * k / R::WIN);  // periodic Hann over the window's support
    for (int b = 0; b < R::NB; ++b) {
      const double th = two_pi * (double)(((R::PADL + k) * b) % R::NFFT) / R::NFFT;  // the angle reduced exactly
      const float v[2] = {(float)(w * cos(th)), (float)(-w * sin(th))};
      for (int c = 0; c < 2; ++c) {
        fwd[(((size_t)c * R::KT + k / 16) * R::NBP + b) * 16 + k % 16] = v[c];
        bwd[(((size_t)c * R::NBT + b / 16) * R::KWP + k) * 16 + b % 16] = v[c];
      }
    }
  }
}

template <class R>
hipError_t forward_r(const float* x, int n, const float* basis, const MrWs& w, int r, bool target, hipStream_t s) {
  const dim3 grid((w.T[r] + R::FT - 1) / R::FT, R::FGY);
  if (target) {
    hipLaunchKernelGGL((mr_fwd_kernel<R, true>), grid, dim3(256), 0, s, x, n, w.T[r], basis, w.ymag[r], w.ylog[r],
                       nullptr, nullptr, w.part[r], w.npart[r]);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return sum_to(w.part[r], (int)(grid.x * grid.y), w.scal + MR_SLOTS * r + MR_SY, 0, s);
  }
  hipLaunchKernelGGL((mr_fwd_kernel<R, false>), grid, dim3(256), 0, s, x, n, w.T[r], basis, w.re[r], w.im[r],
                     w.ymag[r], w.ylog[r], w.part[r], w.npart[r]);
  return hipGetLastError();
}

template <class R>
hipError_t backward_r(const float* basis, const MrWs& w, int r, hipStream_t s) {
  hipLaunchKernelGGL((mr_bwd_kernel<R>), dim3((w.T[r] + R::FT - 1) / R::FT, R::BGY), dim3(256), 0, s, w.T[r], basis + R::TAB,
                     w.re[r], w.im[r], w.ymag[r], w.ylog[r], w.scal + MR_SLOTS * r, w.dF[r]);
  return hipGetLastError();
}

MrGather gather_of(const MrWs& w) {
  MrGather ga;
  for (int r = 0; r < kMrRes; ++r) {
    ga.dF[r] = w.dF[r];
    ga.T[r] = w.T[r];
  }
  return ga;
}

constexpr size_t kMrTabOff[kMrRes] = {0, 2 * MrR0::TAB, 2 * MrR0::TAB + 2 * MrR1::TAB};

}  // namespace

int64_t mrstft_frames(int64_t n, int r) {
  if (n <= kMrMinN) return 0;
  return r == 0 ? frames_of<MrR0>(n) : (r == 1 ? frames_of<MrR1>(n) : (r == 2 ? frames_of<MrR2>(n) : 0));
}

int64_t mrstft_basis_floats() { return (int64_t)(2 * (MrR0::TAB + MrR1::TAB + MrR2::TAB)); }

void mrstft_basis_fill(float* host) {
  fill_tables<MrR0>(host + kMrTabOff[0]);
  fill_tables<MrR1>(host + kMrTabOff[1]);
  fill_tables<MrR2>(host + kMrTabOff[2]);
}

// the pieces of the workspace, each a multiple of 4 floats
MrWs mrstft_ws_map(float* ws, int n, int rows, int64_t* total) {
  constexpr int NBP[kMrRes] = {MrR0::NBP, MrR1::NBP, MrR2::NBP}, KWP[kMrRes] = {MrR0::KWP, MrR1::KWP, MrR2::KWP};
  MrWs w;
  float* p = ws;
  for (int r = 0; r < kMrRes; ++r) {
    const size_t T = (size_t)mrstft_frames(n, r);
    w.T[r] = (int)T;
    w.npart[r] = r == 0 ? npart_of<MrR0>(T) : (r == 1 ? npart_of<MrR1>(T) : npart_of<MrR2>(T));
    w.re[r] = p;
    w.im[r] = w.re[r] + T * NBP[r];
    w.ymag[r] = w.im[r] + T * NBP[r];
    w.ylog[r] = w.ymag[r] + T * NBP[r];
    w.dF[r] = w.ylog[r] + T * NBP[r];
    w.part[r] = w.dF[r] + T * KWP[r];
    p = w.part[r] + 2 * (size_t)w.npart[r];
  }
  w.scal = p;
  p += kMrScalFloats;
  // the point loss (L1 / MSE / SNR) keeps stft.hip's scalars and partials: a view without frames
  w.pt = StftWs{};
  w.pt.T = 0;
  w.pt.npart = (int)up4((size_t)(rows + 255) / 256);
  w.pt.part = p;
  w.pt.scal = w.pt.part + PT_ROWS * (size_t)w.pt.npart;
  w.pt.gchain = w.pt.scal + 32;
  p = w.pt.gchain + up4(rows);
  if (total) *total = (int64_t)(p - ws);
  return w;
}

int64_t mrstft_ws_floats(int n, int rows) {
  int64_t total = 0;
  mrstft_ws_map(nullptr, n, rows, &total);
  return total;
}

hipError_t mrstft_forward(const float* x, int n, const float* basis, const MrWs& w, bool target, hipStream_t s) {
  if (w.T[0] < 1) return hipErrorInvalidValue;
  hipError_t e = forward_r<MrR0>(x, n, basis + kMrTabOff[0], w, 0, target, s);
  if (e == hipSuccess) e = forward_r<MrR1>(x, n, basis + kMrTabOff[1], w, 1, target, s);
  if (e == hipSuccess) e = forward_r<MrR2>(x, n, basis + kMrTabOff[2], w, 2, target, s);
  return e;
}

hipError_t mrstft_finish(const MrWs& w, bool stft, int loss_mode, double alpha, float* loss_out, bool terms,
                         hipStream_t s) {
  constexpr int NB[kMrRes] = {MrR0::NB, MrR1::NB, MrR2::NB}, FT[kMrRes] = {MrR0::FT, MrR1::FT, MrR2::FT};
  constexpr int FGY[kMrRes] = {MrR0::FGY, MrR1::FGY, MrR2::FGY};
  MrFinish f;
  for (int r = 0; r < kMrRes; ++r) {
    f.part[r] = w.part[r];
    f.npart[r] = w.npart[r];
    f.nblk[r] = (w.T[r] + FT[r] - 1) / FT[r] * FGY[r];
    f.T[r] = w.T[r];
    f.NB[r] = NB[r];
  }
  hipLaunchKernelGGL(mr_finish_kernel, dim3(1), dim3(256), 0, s, f, stft ? kMrRes : 0, w.scal, w.pt.scal, loss_mode,
                     alpha, loss_out, terms ? 1 : 0);
  return hipGetLastError();
}

hipError_t mrstft_backward(const float* basis, const MrWs& w, hipStream_t s) {
  if (w.T[0] < 1) return hipErrorInvalidValue;
  hipError_t e = backward_r<MrR0>(basis + kMrTabOff[0], w, 0, s);
  if (e == hipSuccess) e = backward_r<MrR1>(basis + kMrTabOff[1], w, 1, s);
  if (e == hipSuccess) e = backward_r<MrR2>(basis + kMrTabOff[2], w, 2, s);
  return e;
}

hipError_t mrstft_gather(int n, const MrWs& w, float* g, hipStream_t s) {
  hipLaunchKernelGGL(mr_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, gather_of(w), n, g);
  return hipGetLastError();
}

hipError_t mrstft_mix(const float* out, const float* y, int n, int rows, const MrWs& w, int loss_mode, double alpha,
                      float gfac, float* g, hipStream_t s) {
  hipLaunchKernelGGL(mr_mix_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, out, y, n, rows, gather_of(w),
                     w.pt.scal, loss_mode, (float)(1.0 - alpha), (float)alpha, gfac, g);
  return hipGetLastError();
}

}  // namespace siren
