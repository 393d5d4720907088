// The spectral losses (run.py:126-128, :160-169: auraloss.freq.STFTLoss(), auraloss.freq.
// MultiResolutionSTFTLoss(perceptual_weighting=False) and auraloss.time.SNRLoss(), restated from their
// published 0.4.0 definitions) and the loss mix
//   loss = (1 - alpha) {L1 | L_snr | MSE} + alpha {L_stft | L_mrstft}
// for the model output x and the target y, both one sequence of n samples.
//
//   trait   n_fft   hop   win    left zero-pad   bins   frames T     needs
//   SfR     1024    256   1024         0          513   1 + n / 256  n > 512    L_stft
//   MrR0    1024    120    600       212          513   1 + n / 120  n > 1024 \.
//   MrR1    2048    240   1200       424         1025   1 + n / 240  n > 1024  | L_mrstft = (L_0 + L_1 + L_2) / 3
//   MrR2     512     50    240       136          257   1 + n / 50   n > 1024 /.
//   X = stft(x, n_fft, hop, periodic Hann(win) centred in the n_fft frame, center, reflect)
//   x_mag = sqrt(max(re^2 + im^2, 1e-8))
//   L = ||y_mag - x_mag||_F / ||y_mag||_F + mean |log x_mag - log y_mag|
//   L_snr  = -10 log10(sum yc^2 / (sum (xc - yc)^2 + 1e-8) + 1e-8),  xc = x - mean x, yc = y - mean y
//
// Every transform is one instance of StftTraits and runs the same kernels: a GEMM against windowed
// cos / -sin tables (fp64 on the host, rounded to fp32 once) on v_mfma_f32_16x16x4_f32: a small bin's
// log amplifies its error by 1 / x_mag, so no fp16 operands.
//
// K runs over the window's support only.  Taps outside [pad, pad + win) carry a zero window, so the
// table holds the rows k' = tap - pad < KWP = win rounded up to the 16-k group (1024 / 608 / 1200 / 240;
// the rows past win are zero) and frame t reads the padded samples t hop + pad + k'.
//   fwd[c][k' / 16][bin][k' % 16]    bwd[c][bin / 16][k'][bin % 16]    (c: 0 = w cos, 1 = -w sin;
//   bin < NBP = 528 / 528 / 1040 / 272, zero past the last bin); L_mrstft's three one after the other.
// So one wave's 16 bins x 16 k piece is 1 KB contiguous.  As in rff.hip a lane takes k = 4 (l >> 4) + s
// of a 16-k group as its operand of MFMA s for both operands (a permutation of the sum's terms).
// The basis is the MFMA's A operand and the frames its B operand: a lane then holds 4 consecutive
// bins of ONE frame in both the cos and the sin accumulator, forms the magnitude without a lane
// exchange and stores re / im as 16-B pieces.
//
// stft_fwd_kernel<R>: a block owns 16 frames and 4 x WT bin tiles of 16 (WT per wave).  The frames
// are read from the signal staged once in LDS (reflection folded in the staging index), never as a
// [T][n_fft] matrix.  A lane (fr = l & 15, kq = l >> 4) reads the float4 at tap 16 kt + 4 kq of frame fr;
// one ds_read_b128 is served in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and
// the same + 32: a group holds all 16 frames, frames 0-3 and 12-15 at one kq and frames 4-11 at the
// next.  A read is conflict-free when the 16 float4 slots (address / 4 mod 16) of a group differ.
//   SfR (hop 256 = 64 slots = 0 mod 16: one bank for all 16 rows): sig[4940], padded sample q at
//     q + 4 (q / 256): the frames are 260 floats apart, i.e. 4 banks each, the 16 rows x 4 floats of a
//     read covering all 64 banks once.  A float4 never straddles a multiple of 256, so it stays
//     contiguous and 16-B aligned.  Its tables (4.3 MB) stay L2-resident.
//   MrR0 (hop 120 = 30 slots = -2 mod 16): sig[2408], padded sample q at q.  Slot -2 fr + kq: frames
//     fr and fr + 8 share -2 fr, and exactly one of the two sits at the odd kq -- all 16 differ.
//     Every address is a multiple of 4 floats (120, 16, 4).
//   MrR1 (hop 240 = 60 slots = -4 mod 16, 4 distinct values: 4-way): sig[4960], sample q at
//     q + 8 (q / 240): the frame stride becomes 248 floats = 62 slots = -2 mod 16, the case above.
//     q / 240 = fr + kt / 15 (240 = 15 groups of 16), the same for a whole 16-k group, so a float4
//     stays contiguous and 16-B aligned.  Its table (10 MB per layout) does not fit an XCD's 4 MB L2;
//     keeping each table piece for 32 frames per block (half the table traffic, 35 KB of LDS) measured
//     2 % slower than 16 frames per block, so every transform takes 16.
//   MrR2 (hop 50 = 200 B: odd frames are only 8-B aligned, a ds_read_b128 there is replayed): the 16
//     frames get a pitch of their own, sig[16][248] (pitch 62 slots = -2 mod 16, as above), 15.9 KB;
//     the 240 taps of a frame are staged from global memory (L1 / L2 hits: frames overlap 4.8-fold).
// K is accumulated in two interleaved chains (even / odd 16-k groups), summed at the end: fma chains
// of at most 512 / 304 / 608 / 128 terms.
//
// stft_bwd_kernel<R>: dF[T][KWP] = [dRe | dIm][T][2 x NBP] x bwd table.  The B operand (d of one frame,
// 4 consecutive bins per lane) is formed from re / im, the target's magnitudes and the finished
// scalars as it is loaded:
//   d = (x_mag - y_mag) / (sqrt S1 sqrt Sy) + sign(log x_mag - log y_mag) / (x_mag T bins),  0 at the clamp
//   dRe = d re / x_mag, dIm = d im / x_mag
// The gather then sums, per sample, the <= 5 frames that cover it (win / hop <= 5) and the same for its
// reflected images, ascending; L_mrstft adds its transforms in the order 0, 1, 2, each times 1/3 -- no
// float atomics anywhere, two runs are bit-identical.  The scalars are finished in fp64 on the device.
//
// A window (the split step of a micro-batched or data-parallel fit): the forward and the
// backward can run the frame blocks [b0, b1) of the whole signal's ceil(T / 16) alone, the mix (which
// gathers as it goes) the samples [lo, hi) alone.  A block keeps the index it has in the whole-signal
// launch (blockIdx.y * whole gridDim.x + block) for its re / im / dF rows and its partial, and the
// workspace keeps the whole-signal layout; a window starts at a multiple of 16 frames, so the staging
// maps and the alignment arguments above hold as they stand.  spec_window gives the blocks a sample
// range needs (compute) and the ones whose partials it contributes (owned).
#include <math.h>
#include "siren_common.h"
#include "siren_kernels.h"

namespace siren {

namespace {

constexpr float SF_EPS = 1e-8f;
constexpr float MR_THIRD = 1.0f / 3.0f;

template <int NFFT_, int HOP_, int WIN_, int WT_, int BWT_, int PITCH_, int SKEW_>
struct StftTraits {
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
  // guards that only some instances need: an odd number of 16-k groups leaves the second chain's last
  // step empty; backward grids that overhang the taps clamp the overhanging tile's loads and skip its store
  static constexpr bool KT_EVEN = KT % 2 == 0, BWD_EXACT = KT % (4 * BWT_) == 0;
  static_assert(SKEW_ == 0 || HOP_ % 16 == 0, "the skew is constant over a 16-k group");
  static_assert(PITCH_ % 4 == 0 && SKEW_ % 4 == 0 && (PITCH_ || HOP_ % 4 == 0), "16-B aligned float4 reads");
  static_assert(PITCH_ == 0 || PITCH_ >= KWP, "a frame's taps fit its pitch");
  // the frame q / hop that the block's padded sample q >= 0 starts or continues; spelt as a shift
  // where it is one (the compiler cannot see q >= 0)
  static constexpr bool HOP_POW2 = (HOP_ & (HOP_ - 1)) == 0;
  __device__ static __forceinline__ int frame_of(int q) {
    if constexpr (HOP_POW2) return q >> __builtin_ctz(HOP_);
    else return q / HOP_;
  }
  // LDS index of tap 16 kt + fk (fk = 0, 4, 8, 12; + 0..3) of the block's frame f; without a pitch
  // the block's padded sample q sits at q + SKEW frame_of(q)
  __device__ static __forceinline__ int at(int f, int kt, int fk) {
    const int q = HOP_ * f + 16 * kt + fk;
    if constexpr (PITCH_ != 0) return PITCH_ * f + 16 * kt + fk;
    else if constexpr (SKEW_ == 0) return q;
    else if constexpr (HOP_POW2) return q + SKEW_ * frame_of(q);
    else return q + SKEW_ * (f + kt / (HOP_ / 16));   // = frame_of(q), without a division per read
  }
};
//                   n_fft  hop   win  WT BWT pitch skew
using SfR = StftTraits<1024, 256, 1024, 3, 4, 0, 4>;
using MrR0 = StftTraits<1024, 120, 600, 3, 5, 0, 0>;
using MrR1 = StftTraits<2048, 240, 1200, 3, 4, 0, 8>;
using MrR2 = StftTraits<512, 50, 240, 5, 4, 248, 0>;
static_assert(SfR::LDS == 4940 && SfR::SEG == 4864 && SfR::FGY == 3 && SfR::BGY == 4 &&
                  SfR::TAB == (size_t)2 * 1024 * 528 && SfR::PADL == 0 && SfR::KT_EVEN && SfR::BWD_EXACT,
              "the single transform's layout");
static_assert(kStftMinN == SfR::NFFT / 2 && kMrMinN == MrR1::NFFT / 2 && kMrMinN >= MrR0::NFFT / 2 &&
                  kMrMinN >= MrR2::NFFT / 2, "one reflection lands inside the signal");

__device__ __forceinline__ f32x4 sf_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// sample at padded index j of the centred, reflect-padded signal (0 past the padded end: frames >= T);
// n > n_fft / 2, so one reflection lands inside the signal
template <int NFFT>
__device__ __forceinline__ float stft_sample(const float* __restrict__ x, int n, int64_t j) {
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
__global__ __launch_bounds__(256) void stft_fwd_kernel(const float* __restrict__ x, int n, int T,
                                                       const float* __restrict__ basis, float* __restrict__ o0,
                                                       float* __restrict__ o1, const float* __restrict__ ymag,
                                                       const float* __restrict__ ylog, float* __restrict__ part,
                                                       int npart, int blk0, int gx) {
  constexpr int WT = R::WT;
  __shared__ __attribute__((aligned(16))) float sig[R::LDS];
  __shared__ float scratch[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bx = blk0 + blockIdx.x;   // the frame block of the whole signal's gx (a window starts at blk0)
  const int t0 = bx * R::FT;
  const int64_t j0 = (int64_t)t0 * R::HOP + R::PADL;
  if constexpr (R::PITCH != 0) {
    for (int e = tid; e < R::FT * R::KWP; e += 256) {
      const int f = e / R::KWP, u = e - f * R::KWP;
      sig[R::PITCH * f + u] = stft_sample<R::NFFT>(x, n, j0 + f * R::HOP + u);
    }
  } else {
    for (int q = tid; q < R::SEG; q += 256) sig[q + R::SKEW * R::frame_of(q)] = stft_sample<R::NFFT>(x, n, j0 + q);
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
  // the next 16-k group's table pieces travel under this group's MFMAs
  float4 bcA[WT], bsA[WT], bcB[WT], bsB[WT];
  load_b(0, bcA, bsA);
  for (int kt = 0; kt < R::KT; kt += 2) {
    const bool odd = R::KT_EVEN || kt + 1 < R::KT;
    if (odd) load_b(kt + 1, bcB, bsB);
    step(kt, bcA, bsA, ac[0], as[0]);
    if (kt + 2 < R::KT) load_b(kt + 2, bcA, bsA);
    if (odd) step(kt + 1, bcB, bsB, ac[1], as[1]);
  }

  // lane: frame t0 + fr, bins (bt0 + j) 16 + fk + r
  const int t = t0 + fr;
  float s1 = 0.f, sl = 0.f;
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    if (bt0 + j >= R::NBT || t >= T) continue;
    const f32x4 re = ac[0][j] + ac[1][j], im = as[0][j] + as[1][j];
    const size_t o = (size_t)t * R::NBP + (bt0 + j) * 16 + fk;
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
    const int blk = blockIdx.y * gx + bx;
    part[(size_t)PT_S1 * npart + blk] = s1;
    part[(size_t)PT_SL * npart + blk] = sl;
  }
}

template <class R>
__global__ __launch_bounds__(256) void stft_bwd_kernel(int T, const float* __restrict__ basisT,
                                                       const float* __restrict__ re, const float* __restrict__ im,
                                                       const float* __restrict__ ymag,
                                                       const float* __restrict__ ylog,
                                                       const float* __restrict__ scal, float* __restrict__ dF,
                                                       int blk0) {
  constexpr int BWT = R::BWT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fk = 4 * (lane >> 4);
  const int t = (blk0 + blockIdx.x) * R::FT + fr;
  const bool valid = t < T;
  const int nt0 = (blockIdx.y * 4 + wave) * BWT;
  const float c1 = scal[SC_C1], c2 = scal[SC_C2];
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
  auto load_b = [&](int bg, float4 (&bc)[BWT], float4 (&bs)[BWT]) {
#pragma unroll
    for (int j = 0; j < BWT; ++j) {
      const int nt = R::BWD_EXACT || nt0 + j < R::KT ? nt0 + j : R::KT - 1;   // a tile past the last: not stored
      const size_t o = ((size_t)bg * R::KWP + nt * 16 + fr) * 16 + fk;
      bc[j] = *(const float4*)(basisT + o);
      bs[j] = *(const float4*)(basisT + (size_t)R::NBT * R::KWP * 16 + o);
    }
  };
  auto step = [&](const float (&dre)[4], const float (&dim)[4], const float4 (&bc)[BWT], const float4 (&bs)[BWT],
                  f32x4 (&a)[BWT]) {
#pragma unroll
    for (int j = 0; j < BWT; ++j) {
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
      if (!R::BWD_EXACT && nt0 + j >= R::KT) continue;
      const f32x4 v = acc[0][j] + acc[1][j];
      *(float4*)(dF + (size_t)t * R::KWP + (nt0 + j) * 16 + fk) = float4{v[0], v[1], v[2], v[3]};
    }
  }
}

// contributions of padded index j: the frames t hop + pad <= j < t hop + pad + win, t < T, ascending
template <class R>
__device__ __forceinline__ float gather_j(const float* __restrict__ dF, int64_t j, int T) {
  const int64_t a = j - R::PADL;   // tap 0 of frame t sits at a = t hop
  if constexpr (R::PADL != 0)
    if (a < 0) return 0.f;
  const int64_t tlo = a < R::WIN ? 0 : (a - R::WIN) / R::HOP + 1;
  int64_t thi = a / R::HOP;
  if (thi > T - 1) thi = T - 1;
  float s = 0.f;
  for (int64_t t = tlo; t <= thi; ++t) s += dF[t * R::KWP + (a - t * R::HOP)];
  return s;
}
// dL/dx_i of one transform: sample i itself (padded index i + n_fft / 2), its image in the left
// reflection (n_fft / 2 - i, i in 1..n_fft / 2) and in the right one (2 (n - 1) - i + n_fft / 2, i in
// n - 1 - n_fft / 2..n - 2), in that order
template <class R>
__device__ __forceinline__ float gather_sample(const float* __restrict__ dF, int i, int n, int T) {
  constexpr int H = R::NFFT / 2;
  float s = gather_j<R>(dF, (int64_t)i + H, T);
  if (i >= 1 && i <= H) s += gather_j<R>(dF, H - i, T);
  if (i <= n - 2 && i >= n - H - 1) s += gather_j<R>(dF, 2 * (int64_t)(n - 1) - i + H, T);
  return s;
}

// the two gathers: dL_stft/dx_i, and dL_mrstft/dx_i = the three transforms in the order 0, 1, 2, each times 1/3
struct GatherSf {
  const float* dF;
  int T;
  __device__ __forceinline__ float operator()(int i, int n) const { return gather_sample<SfR>(dF, i, n, T); }
};
struct GatherMr {
  const float* dF[kMrRes];
  int T[kMrRes];
  __device__ __forceinline__ float operator()(int i, int n) const {
    float s = MR_THIRD * gather_sample<MrR0>(dF[0], i, n, T[0]);
    s += MR_THIRD * gather_sample<MrR1>(dF[1], i, n, T[1]);
    s += MR_THIRD * gather_sample<MrR2>(dF[2], i, n, T[2]);
    return s;
  }
};
GatherSf gather_sf(const SpecWs& w) { return GatherSf{w.r[0].dF, w.r[0].T}; }
GatherMr gather_mr(const SpecWs& w) {
  GatherMr ga;
  for (int r = 0; r < kMrRes; ++r) {
    ga.dF[r] = w.r[r].dF;
    ga.T[r] = w.r[r].T;
  }
  return ga;
}

template <class G>
__global__ void stft_gather_kernel(G ga, int n, float* __restrict__ g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) g[i] = ga(i, n);
}

// g = (1 - alpha) g_point + alpha gather over the valid rows, 0 on pad rows (pscal: the point loss's scalars);
// rows [lo, rows) of the batch
template <class G>
__global__ void loss_mix_kernel(const float* __restrict__ out, const float* __restrict__ y, int n, int lo, int rows,
                                G ga, const float* __restrict__ pscal, int loss_mode, float wp, float ws, float gfac,
                                float* __restrict__ g) {
  const int i = lo + blockIdx.x * blockDim.x + threadIdx.x;
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
    if (ws != 0.f) v += ws * ga(i, n);
  }
  g[i] = v;
}

// The point loss's |err| (loss_mode 1) or err^2 per 256 samples of a signal whose `out` is already
// written: head_loss_kernel's err and its block reduction (block_sum2_max keeps block_sum's tree), so
// the partials are those of a one-batch step over the same out, bit for bit
__global__ void point_partials_kernel(const float* __restrict__ out, const float* __restrict__ y, int n,
                                      int loss_mode, float* __restrict__ part) {
  __shared__ float scratch[4];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  float e2 = 0.f;
  if (i < n) {
    const float err = out[i] - y[i];
    e2 = loss_mode == 1 ? fabsf(err) : err * err;
  }
  const float se = block_sum(e2, scratch);
  if (threadIdx.x == 0) part[blockIdx.x] = se;
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

// fp64 sum of cnt fp32 partials by one block of 256 in a fixed order (sh: 256 doubles); valid in thread 0
__device__ __forceinline__ double block_total(const float* p, int cnt, double* sh) {
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int k = tid; k < cnt; k += 256) a += (double)p[k];
  __syncthreads();
  sh[tid] = a;
  __syncthreads();
  double s = 0.0;
  if (tid == 0)
    for (int k = 0; k < 256; ++k) s += sh[k];
  return s;
}

// one transform's finished scalars from its nblk partials: S1, sum|dlog| -> L (returned, valid in
// thread 0), c1 = 1 / (sqrt S1 sqrt Sy), c2 = 1 / (T bins), stored in sc[SC_S1..SC_C2]
__device__ __forceinline__ double finish_term(const float* part, int npart, int nblk, int T, int bins, float* sc,
                                              double* sh) {
  const double S1 = block_total(part + (size_t)PT_S1 * npart, nblk, sh);
  const double SL = block_total(part + (size_t)PT_SL * npart, nblk, sh);
  double l = 0.0;
  if (threadIdx.x == 0) {
    const double Sy = (double)sc[SC_SY];
    const double r1 = sqrt(S1), ry = sqrt(Sy), cnt = (double)T * bins;
    l = r1 / ry + SL / cnt;
    sc[SC_S1] = (float)S1;
    sc[SC_SL] = (float)SL;
    sc[SC_LSTFT] = (float)l;
    sc[SC_C1] = (S1 > 0.0 && Sy > 0.0) ? (float)(1.0 / (r1 * ry)) : 0.f;
    sc[SC_C2] = (float)(1.0 / cnt);
  }
  return l;
}

// The two finish kernels stay two: the single one mixes the fp64 point loss in the launch that forms
// it, the multi-resolution one reads it back as fp32 from SC_LPOINT -- one kernel for both would change
// the low bits of one path's loss history.
//
// the finished scalars (one block, fp64 sums of the fp32 partials in a fixed order):
//   nstft > 0: the single transform's term (finish_term)
//   loss_mode 2: L_snr and the gradient factor; 0 / 1: the mean of sse_part's sum (MSE / L1); -1: none
//   loss = (1 - alpha) point + alpha L_stft (loss_mode -1: L_stft), fp32, also to loss_out[0]
__global__ __launch_bounds__(256) void loss_finish_kernel(float* __restrict__ scal, const float* __restrict__ part,
                                                          int npart, int nstft, int nsnr,
                                                          const float* __restrict__ sse_part, int nsum,
                                                          int loss_mode, double alpha, double n_total, int T,
                                                          float* __restrict__ loss_out) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  double lstft = 0.0, lpoint = 0.0;
  if (nstft > 0) lstft = finish_term(part, npart, nstft, T, SfR::NB, scal, sh);
  if (loss_mode == 2) {
    const double Syc = block_total(part + (size_t)PT_SYC * npart, nsnr, sh) +
                       block_total(part + (size_t)PT_SYC_LO * npart, nsnr, sh);
    const double Sr = block_total(part + (size_t)PT_SR * npart, nsnr, sh) +
                      block_total(part + (size_t)PT_SR_LO * npart, nsnr, sh);
    if (tid == 0) {
      const double eps = 1e-8, q = Syc / (Sr + eps);
      lpoint = -10.0 * log10(q + eps);
      scal[SC_SYC] = (float)Syc;
      scal[SC_SR] = (float)Sr;
      scal[SC_LSNR] = (float)lpoint;
      scal[SC_FSNR] = (float)((10.0 / log(10.0)) * (q / (q + eps)) * (2.0 / (Sr + eps)));
    }
  } else if (loss_mode >= 0) {
    const double se = block_total(sse_part, nsum, sh);
    if (tid == 0) lpoint = se / n_total;
  }
  if (tid == 0) {
    const double loss = loss_mode < 0 ? lstft : (1.0 - alpha) * lpoint + alpha * lstft;
    scal[SC_LPOINT] = (float)lpoint;
    scal[SC_LOSS] = (float)loss;
    if (loss_out) loss_out[0] = (float)loss;
  }
}

struct MrFinish {
  const float* part[kMrRes];
  int npart[kMrRes], nblk[kMrRes], T[kMrRes], NB[kMrRes];
};
// per resolution finish_term into scal[MR_SLOTS r + ...], then L_mrstft = (L_0 + L_1 + L_2) / 3 and
// loss = (1 - alpha) point + alpha L_mrstft (loss_mode -1: L_mrstft), the point loss from
// loss_finish_kernel's scalars.  nres 0: no spectral term (loss = point).
// loss_out[0] <- loss; terms: loss_out[1..3] <- L_0, L_1, L_2
__global__ __launch_bounds__(256) void mr_finish_kernel(MrFinish f, int nres, float* __restrict__ scal,
                                                        const float* __restrict__ pscal, int loss_mode, double alpha,
                                                        float* __restrict__ loss_out, int terms) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  double lsum = 0.0;
  for (int r = 0; r < nres; ++r) {
    const double l = finish_term(f.part[r], f.npart[r], f.nblk[r], f.T[r], f.NB[r], scal + MR_SLOTS * r, sh);
    if (tid == 0) {
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

// what the host needs of a trait: the sizes, the table fill and the two launches
struct ResInfo {
  int hop, nb, nbp, kwp, ft, fgy, nfft, win;
  size_t tab;
  void (*fill)(float* fwd);
  // b0, b1: the frame blocks [b0, b1) of the whole signal's that run (a window; the target side runs them all)
  hipError_t (*forward)(const float* x, int n, const float* basis, const SpecRes& q, bool target, int b0, int b1,
                        hipStream_t s);
  hipError_t (*backward)(const float* basis, const SpecRes& q, int b0, int b1, hipStream_t s);
  int fblocks(int64_t T) const { return (int)((T + ft - 1) / ft); }        // frame blocks of the whole signal
  int blocks(int64_t T) const { return fblocks(T) * fgy; }                 // forward blocks = partials per row
};

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
hipError_t forward_r(const float* x, int n, const float* basis, const SpecRes& q, bool target, int b0, int b1,
                     hipStream_t s) {
  const int gx = (q.T + R::FT - 1) / R::FT;
  if (target) {
    const dim3 grid(gx, R::FGY);
    hipLaunchKernelGGL((stft_fwd_kernel<R, true>), grid, dim3(256), 0, s, x, n, q.T, basis, q.ymag, q.ylog, nullptr,
                       nullptr, q.part, q.npart, 0, gx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return sum_to(q.part + (size_t)PT_S1 * q.npart, (int)(grid.x * grid.y), q.scal + SC_SY, 0, s);
  }
  if (b0 < 0 || b1 > gx || b0 > b1) return hipErrorInvalidValue;
  if (b0 == b1) return hipSuccess;   // an empty window
  hipLaunchKernelGGL((stft_fwd_kernel<R, false>), dim3(b1 - b0, R::FGY), dim3(256), 0, s, x, n, q.T, basis, q.re,
                     q.im, q.ymag, q.ylog, q.part, q.npart, b0, gx);
  return hipGetLastError();
}

template <class R>
hipError_t backward_r(const float* basis, const SpecRes& q, int b0, int b1, hipStream_t s) {
  if (b0 < 0 || b1 > (q.T + R::FT - 1) / R::FT || b0 > b1) return hipErrorInvalidValue;
  if (b0 == b1) return hipSuccess;
  hipLaunchKernelGGL((stft_bwd_kernel<R>), dim3(b1 - b0, R::BGY), dim3(256), 0, s, q.T, basis + R::TAB, q.re, q.im,
                     q.ymag, q.ylog, q.scal, q.dF, b0);
  return hipGetLastError();
}

template <class R>
constexpr ResInfo info_of() {
  return {R::HOP, R::NB, R::NBP, R::KWP, R::FT, R::FGY, R::NFFT, R::WIN, R::TAB, fill_tables<R>, forward_r<R>,
          backward_r<R>};
}
// a loss's transforms, their tables one after the other
const ResInfo kSfRes[1] = {info_of<SfR>()};
const ResInfo kMrResInfo[kMrRes] = {info_of<MrR0>(), info_of<MrR1>(), info_of<MrR2>()};
const ResInfo* res_of(SpecLoss k) { return k == SPEC_MRSTFT ? kMrResInfo : kSfRes; }
int nres_of(SpecLoss k) { return k == SPEC_MRSTFT ? kMrRes : 1; }

// re .. dF of one transform at p; returns the float after them
float* map_res(SpecRes& q, const ResInfo& ri, float* p, size_t T) {
  q.T = (int)T;
  q.re = p;
  q.im = q.re + T * ri.nbp;
  q.ymag = q.im + T * ri.nbp;
  q.ylog = q.ymag + T * ri.nbp;
  q.dF = q.ylog + T * ri.nbp;
  return q.dF + T * ri.kwp;
}
// the point loss's pieces at p; returns the float after them
float* map_point(PointWs& pt, float* p, int npart, int rows) {
  pt.npart = npart;
  pt.part = p;
  pt.scal = pt.part + PT_ROWS * (size_t)npart;
  pt.gchain = pt.scal + 32;
  return pt.gchain + up4(rows);
}

}  // namespace

int64_t spec_frames(SpecLoss k, int64_t n, int r) {
  if (n <= (k == SPEC_MRSTFT ? kMrMinN : kStftMinN) || r < 0 || r >= nres_of(k)) return 0;
  return 1 + n / res_of(k)[r].hop;
}

int64_t spec_basis_floats(SpecLoss k) {
  size_t f = 0;
  for (int r = 0; r < nres_of(k); ++r) f += 2 * res_of(k)[r].tab;
  return (int64_t)f;
}

void spec_basis_fill(SpecLoss k, float* host) {
  for (int r = 0; r < nres_of(k); ++r) {
    res_of(k)[r].fill(host);
    host += 2 * res_of(k)[r].tab;
  }
}

// the pieces of the workspace, each a multiple of 4 floats
SpecWs spec_ws_map(SpecLoss k, float* ws, int n, int rows, int64_t* total) {
  const ResInfo* ri = res_of(k);
  const int bands = (rows + 255) / 256;
  SpecWs w = {};
  w.loss = k;
  w.nres = nres_of(k);
  float* p = ws;
  if (k == SPEC_STFT) {
    // one [PT_ROWS][npart] block and one scal[32] serve the transform and the point loss
    const size_t T = (size_t)spec_frames(k, n, 0);
    const int blocks = ri[0].blocks((int64_t)T);
    p = map_res(w.r[0], ri[0], p, T);
    p = map_point(w.pt, p, (int)up4(blocks > bands ? blocks : bands), rows);
    w.r[0].part = w.pt.part;
    w.r[0].npart = w.pt.npart;
    w.r[0].scal = w.scal = w.pt.scal;
  } else {
    // per transform its own [2][npart_r], then scal[kMrScalFloats] (MR_SLOTS each), then the point loss
    for (int r = 0; r < kMrRes; ++r) {
      const size_t T = (size_t)spec_frames(k, n, r);
      w.r[r].part = map_res(w.r[r], ri[r], p, T);
      w.r[r].npart = (int)up4((size_t)ri[r].blocks((int64_t)T));
      p = w.r[r].part + 2 * (size_t)w.r[r].npart;
    }
    w.scal = p;
    for (int r = 0; r < kMrRes; ++r) w.r[r].scal = w.scal + MR_SLOTS * r;
    p = map_point(w.pt, p + kMrScalFloats, (int)up4((size_t)bands), rows);
  }
  if (total) *total = (int64_t)(p - ws);
  return w;
}

int spec_frame_blocks(SpecLoss k, int64_t n, int r) {
  const int64_t T = spec_frames(k, n, r);
  return T > 0 ? res_of(k)[r].fblocks(T) : 0;
}

int spec_grid_y(SpecLoss k, int r) { return r >= 0 && r < nres_of(k) ? res_of(k)[r].fgy : 0; }

// The frame blocks of transform r that the samples [lo, hi) of an n-sample signal need and own.
// Frame t covers the padded indices j with t hop <= j - pad < t hop + win.  compute: every block with
// a frame that covers i + n_fft / 2 or one of i's two reflected images (gather_sample's) for an i in
// [lo, hi) -- what the gather of dL/dx_i reads, hence what the forward and the backward of that range
// must have run.  owned: the blocks whose first frame t0 has min(t0 hop, n - 1) in [lo, hi); that
// sample is monotone in the block, so any partition of [0, n) partitions the blocks, and frame t0
// covers its image (win / 2 taps in), so compute contains owned.  A block is 16 frames: a window starts
// at a multiple of 16 frames and every staging map of the kernels holds unchanged.
void spec_window(SpecLoss k, int r, int n, int lo, int hi, int compute[2], int owned[2]) {
  const ResInfo& ri = res_of(k)[r];
  const int64_t T = spec_frames(k, n, r), H = ri.nfft / 2, pad = (ri.nfft - ri.win) / 2;
  const int nblk = ri.fblocks(T);
  int64_t fmin = T, fmax = -1;   // covering frames
  auto cover = [&](int64_t j0, int64_t j1) {   // the padded indices [j0, j1]
    const int64_t a0 = j0 - pad < 0 ? 0 : j0 - pad, a1 = j1 - pad;
    if (j0 > j1 || a1 < 0) return;
    const int64_t tlo = a0 < ri.win ? 0 : (a0 - ri.win) / ri.hop + 1;
    const int64_t thi = a1 / ri.hop > T - 1 ? T - 1 : a1 / ri.hop;
    if (tlo > thi) return;
    if (tlo < fmin) fmin = tlo;
    if (thi > fmax) fmax = thi;
  };
  if (lo < hi) {
    const int64_t last = hi - 1, N1 = n - 1;
    cover(lo + H, last + H);
    cover(H - (last < H ? last : H), H - (lo > 1 ? lo : 1));                              // i in 1 .. n_fft / 2
    cover(2 * N1 - (last < N1 - 1 ? last : N1 - 1) + H, 2 * N1 - (lo > N1 - H ? lo : N1 - H) + H);  // n-1-H .. n-2
  }
  compute[0] = fmax < 0 ? 0 : (int)(fmin / ri.ft);
  compute[1] = fmax < 0 ? 0 : (int)(fmax / ri.ft) + 1;
  const int64_t bs = (int64_t)ri.ft * ri.hop;   // samples between two blocks' first frames
  auto first_at = [&](int64_t x) {   // the first block whose min(t0 hop, n - 1) >= x
    const int64_t b = (x + bs - 1) / bs;
    return x > n - 1 || b > nblk ? nblk : (int)b;
  };
  owned[0] = first_at(lo);
  owned[1] = first_at(hi);
}

// win: per transform the frame blocks [win[2 r], win[2 r + 1]) that run; null: all of them
hipError_t spec_forward(const float* x, int n, const float* basis, const SpecWs& w, bool target, hipStream_t s,
                        const int* win) {
  if (w.r[0].T < 1) return hipErrorInvalidValue;
  const ResInfo* ri = res_of((SpecLoss)w.loss);
  hipError_t e = hipSuccess;
  for (int r = 0; r < w.nres && e == hipSuccess; ++r) {
    e = ri[r].forward(x, n, basis, w.r[r], target, win ? win[2 * r] : 0, win ? win[2 * r + 1] : ri[r].fblocks(w.r[r].T),
                      s);
    basis += 2 * ri[r].tab;
  }
  return e;
}

hipError_t spec_backward(const float* basis, const SpecWs& w, hipStream_t s, const int* win) {
  if (w.r[0].T < 1) return hipErrorInvalidValue;
  const ResInfo* ri = res_of((SpecLoss)w.loss);
  hipError_t e = hipSuccess;
  for (int r = 0; r < w.nres && e == hipSuccess; ++r) {
    e = ri[r].backward(basis, w.r[r], win ? win[2 * r] : 0, win ? win[2 * r + 1] : ri[r].fblocks(w.r[r].T), s);
    basis += 2 * ri[r].tab;
  }
  return e;
}

hipError_t point_partials(const float* out, const float* y, int n, int loss_mode, const SpecWs& w, hipStream_t s) {
  hipLaunchKernelGGL(point_partials_kernel, dim3((n + 255) / 256), dim3(256), 0, s, out, y, n, loss_mode,
                     w.pt.part + (size_t)PT_SSE * w.pt.npart);
  return hipGetLastError();
}

hipError_t snr_sums(const float* x, const float* y, int n, const SpecWs& w, hipStream_t s) {
  const int nblk = (n + 255) / 256;
  hipLaunchKernelGGL(snr_sums1_kernel, dim3(nblk), dim3(256), 0, s, x, y, n, w.pt.part, w.pt.npart);
  hipLaunchKernelGGL(snr_sums2_kernel, dim3(nblk), dim3(256), 0, s, x, y, n, w.pt.part, w.pt.npart, nblk, w.pt.scal);
  return hipGetLastError();
}

hipError_t loss_finish(const SpecWs& w, int n, const float* sse_part, int nsum, int loss_mode, double alpha,
                       double n_total, bool stft, float* loss_out, hipStream_t s) {
  const int nstft = stft ? kSfRes[0].blocks(w.r[0].T) : 0;
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, s, w.pt.scal, w.pt.part, w.pt.npart, nstft,
                     (n + 255) / 256, sse_part, nsum, loss_mode, alpha, n_total, w.r[0].T, loss_out);
  return hipGetLastError();
}

hipError_t mrstft_finish(const SpecWs& w, bool stft, int loss_mode, double alpha, float* loss_out, bool terms,
                         hipStream_t s) {
  MrFinish f;
  for (int r = 0; r < kMrRes; ++r) {
    f.part[r] = w.r[r].part;
    f.npart[r] = w.r[r].npart;
    f.nblk[r] = kMrResInfo[r].blocks(w.r[r].T);
    f.T[r] = w.r[r].T;
    f.NB[r] = kMrResInfo[r].nb;
  }
  hipLaunchKernelGGL(mr_finish_kernel, dim3(1), dim3(256), 0, s, f, stft ? kMrRes : 0, w.scal, w.pt.scal, loss_mode,
                     alpha, loss_out, terms ? 1 : 0);
  return hipGetLastError();
}

hipError_t spec_gather(int n, const SpecWs& w, float* g, hipStream_t s) {
  const dim3 grid((n + 255) / 256), block(256);
  if (w.loss == SPEC_MRSTFT) hipLaunchKernelGGL(stft_gather_kernel<GatherMr>, grid, block, 0, s, gather_mr(w), n, g);
  else hipLaunchKernelGGL(stft_gather_kernel<GatherSf>, grid, block, 0, s, gather_sf(w), n, g);
  return hipGetLastError();
}

hipError_t loss_mix(const float* out, const float* y, int n, int rows, const SpecWs& w, int loss_mode, double alpha,
                    float gfac, float* g, hipStream_t s, int lo) {
  if (lo >= rows) return hipSuccess;
  const dim3 grid((rows - lo + 255) / 256), block(256);
  const float wp = (float)(1.0 - alpha), wsp = (float)alpha;
  if (w.loss == SPEC_MRSTFT)
    hipLaunchKernelGGL(loss_mix_kernel<GatherMr>, grid, block, 0, s, out, y, n, lo, rows, gather_mr(w), w.pt.scal,
                       loss_mode, wp, wsp, gfac, g);
  else
    hipLaunchKernelGGL(loss_mix_kernel<GatherSf>, grid, block, 0, s, out, y, n, lo, rows, gather_sf(w), w.pt.scal,
                       loss_mode, wp, wsp, gfac, g);
  return hipGetLastError();
}

}  // namespace siren
