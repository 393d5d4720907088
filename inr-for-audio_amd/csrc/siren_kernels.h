// Internal host-side launchers for the SIREN gfx950 kernels (not the public C-ABI;
// that lives in include/siren_hip.h and capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace siren {

typedef _Float16 h16;  // activation / weight-shadow / gradient storage (fp16)

// NT_FWD_SNAKE / NT_FWD_TANH: Linear + Snake / Tanh forward epilogues; NT_DX_SNAKE: dX into
// a Snake layer (derivative D and d/da E of the layer below), SURVEY §8 f3
// NT_DX0_SNAKE: dX into a Linear + Snake first layer (first_linear=True): dz = acc * D0, partials
// of db0, dW0 (x t_j) and da0 = sum acc * E0
// NT_FWD_HB: the last hidden SineLayer fused with the head, the loss gradient and the head backward
// (training only): writes dZ_L x S instead of Y_L / C_L (see gemm_nt.hip)
// NT_FWD_HB_SNAKE / NT_FWD_HB_TANH: the same for a Linear + Snake / Linear + Tanh last layer
// (run.py:30's default train() stack ends in Snake layers)
enum NtMode { NT_FWD = 0, NT_DX = 1, NT_DX0 = 2, NT_FWD_SNAKE = 3, NT_FWD_TANH = 4, NT_DX_SNAKE = 5,
              NT_DX0_SNAKE = 6, NT_FWD_HB = 7, NT_FWD_HB_SNAKE = 8, NT_FWD_HB_TANH = 9 };
constexpr bool nt_is_hb(int m) { return m == NT_FWD_HB || m == NT_FWD_HB_SNAKE || m == NT_FWD_HB_TANH; }
constexpr bool nt_is_fwd(int m) { return m == NT_FWD || m == NT_FWD_SNAKE || m == NT_FWD_TANH || nt_is_hb(m); }
// forward modes that evaluate a Snake (they stage a and 1/a in LDS)
constexpr bool nt_is_snake_fwd(int m) { return m == NT_FWD_SNAKE || m == NT_FWD_HB_SNAKE; }

// The siren_set_option knobs (include/siren_hip.h enum siren_option), one member per option:
// process-global and unsynchronised.  capi.hip's option table holds each one's default and
// accepted values and is the only writer; the launchers read tuning().x.
struct Tuning {
  int nt_tile, tn_tile;  // forced GEMM tile edge (0 = automatic, 128, 256)
  int nt_pipe, tn_pipe;  // 256x256 K-loop variant (-1 = automatic = 4)
  int nt_grid;           // persistent NT grid size (0 = one block per CU)
  int nt_diag;           // measurement-only NT ablation bits (SIREN_DIAG builds)
  int nt_queue;          // dynamic tile queue: 0 off, 1 forward modes, 2 every ping-pong mode
  int head_fuse;         // siren_train_step runs the last layer as NT_FWD_HB* when it can
  int hb_fault;          // hand-off fault hook (SIREN_DIAG builds)
  int kan_general;       // grid_size 5 runs the any-grid-size KAN kernels (tests and measurement)
};
Tuning& tuning();

struct NtParams {
  const h16* X;  // [M][K]
  const h16* W;  // [N][K]
  int M, N, K;
  int ld;         // row stride of the [M][*] operands and outputs: gemm_nt sets it (= N; column
                  // windows of a layer wider than 1024 keep the layer's width)
  int tile;       // 128 or 256 (nt_choose_tile): partials are per tile-row / tile-column
  float omega;  // FWD: this layer's omega; DX: omega of the layer below; DX0: omega_0
  // NT_FWD
  const float* bias;    // [N]
  h16* Y;              // [M][N]
  h16* C;              // [M][N]  sine: cos; Snake: dY/dz = 1 + sin(2az); Tanh: 1 - y^2
  h16* E;              // [M][N]  Snake only: dY/da = (z sin(2az) - sin^2(az)/a) / a
  const float* act_a;  // [N]     Snake only: a (per output column)
  const float* head_w;  // [N]          (HEAD only)
  float* head_part;     // [N/128][M]   (HEAD only)
  // NT_DX / NT_DX0
  const h16* Cprev;    // [M][N]  cos of the layer below (NT_DX); D of a Snake / 1-y^2 of a Tanh
  const h16* Eprev;    // [M][N]  NT_DX_SNAKE: E of the Snake layer below
  h16* dZ;             // [M][N]  (NT_DX)
  float* colsum_part;   // NT_DX: [M/128][N];  NT_DX0: [M/128][1+in][N];  NT_DX_SNAKE: [M/128][2][N];
                        // NT_DX0_SNAKE: [M/128][2+in][N] (db0, dW0[:, j], da0)
  // NT_DX0 (Cprev = cos of the first layer)
  const float* t;       // [M][in]
  int in_dim;
  const float* gscale;  // NT_DX / NT_DX0: {S, 1/S} -- column partials are multiplied by 1/S
                        // (null = unscaled)
  int diag;             // SIREN_OPT_NT_DIAG ablation bits (SIREN_DIAG measurement builds only)
  // ping-pong K-loop only: caller-owned tile-queue counter set of kTileqInts ints (null = the
  // static walk b, b + G, ...); gemm_nt zeroes it on the stream before each queue launch
  int* tileq;
  // NT_FWD_HB* (with head_w / head_part; gscale = {S, 1/S} set beforehand by grad_scale_bound, or
  // for a Snake last layer by grad_scale from the previous launch's max|g|; dZ = dZ_L x S;
  // colsum_part [M/256][2][N] = partials of db_L and dw_head, Snake [M/256][3][N] + da_L):
  // head_loss's inputs and outputs for the band's rows
  const float* target;  // [M]
  const float* b_head;  // [1]
  float* out;           // [M]
  float* g;             // [M] dLoss/d(head linear output)
  float* sse_part;      // [M/256]
  float* gsum_part;     // [M/256]
  int n_valid, loss_mode;
  float gfac, head_omega;
  float* gmax_part;     // [M/256] max|g| per band (NT_FWD_HB*; null = not written)
  // NT_FWD_HB*: a hand-off wait that gives up (spin_limit polls) adds 1 here (GuardState::stalls;
  // null = only the NaN partial); hb_fault: SIREN_OPT_HB_FAULT injection (SIREN_DIAG builds only)
  int* stall;
  int spin_limit, hb_fault;
};
constexpr int kTileqInts = 768;  // == SIREN_TILEQ_INTS (include/siren_hip.h)

int nt_choose_tile(int M, int N);
hipError_t gemm_nt(int mode, bool head, const NtParams& p, hipStream_t s);
// the forward (NT_FWD, no head) with its epilogue under the next tile's MFMAs: one wave per SIMD,
// 128x256 tiles, K / 64 in {4, 8, 16}, N / 256 in {1, 2, 4} (gemm_nt1.hip; SIREN_OPT_NT_PIPE 5)
bool gemm_nt_one_ok(const NtParams& p);
hipError_t gemm_nt_one(const NtParams& p, int grid, int diag, bool overlap, hipStream_t s);  // pipe 5 / 7
// the forward (NT_FWD, no head) with one wave per SIMD on 256x256 tiles, BK 32, 4-stage ring:
// K % 128 == 0, N / 256 in {1, 2, 4} (gemm_nt2.hip; SIREN_OPT_NT_PIPE 6)
bool gemm_nt_big_ok(const NtParams& p);
hipError_t gemm_nt_big(const NtParams& p, int grid, int diag, hipStream_t s);
// NT_FWD_HB is available for this shape under the current tile / K-loop settings
// also false when the fused launch's grid could not be co-resident (occupancy x CUs < grid)
bool gemm_nt_head_fusable(int M, int N, hipStream_t s, int mode = NT_FWD_HB);
struct TnParams {
  const h16* Y;   // [R][Hin]   layer input (A role: dW column index k)
  const h16* dZ;  // [R][Hout]  layer pre-activation gradient (B role: dW row index o)
  int R, Hin, Hout;
  int splits;
  int tile;        // 128 or 256 (tn_choose_tile); dw_reduce must be given the same value
  float* slab;     // [splits][Hout*Hin] fp32 in MFMA-native order (see dw_reduce)
};

int tn_choose_tile(int R, int Hin, int Hout);
hipError_t gemm_tn_dw(const TnParams& p, hipStream_t s);
// grad[o][k] (+)= sum_s slab[s]  (grad row-major [Hout][Hin])
// (scaled by gscale[1] = 1/S when gscale is non-null: dZ carries the backward scale S)
hipError_t dw_reduce(const float* slab, int splits, int Hin, int Hout, int tile, float* grad,
                     int accumulate, const float* gscale, hipStream_t s);

// elementwise / reduction kernels (elementwise.hip)
hipError_t coords_fill(float* t, int64_t rows, int64_t offset, int64_t n_total, hipStream_t s);
hipError_t coords_fill_grid(float* xy, int64_t rows, int64_t offset, int64_t height, int width, hipStream_t s);

// fp16 backward range guard (include/siren_hip.h siren_guard)
struct GuardState {
  int32_t flag, headroom, clean, overflows, headroom0;
  int32_t stalls;  // fused last layer: timed-out hand-off waits (sticky; the host clears it)
};
constexpr int kHeadroomDefault = 6;      // grad_scale target exponent without a guard
constexpr int kHeadroomDrop = 4;         // per rejected step (S / 16)
constexpr int kHeadroomMin = -14;        // below this a non-finite gradient is passed through
constexpr int kHeadroomGrowAfter = 1000; // clean steps before headroom grows back by one
// true when the step's gradients hold a non-finite value, the loss is finite (so it is the
// fp16 dZ storage that overflowed, not a diverged fit) and the headroom can still drop
__device__ __forceinline__ bool guard_overflow(const GuardState* g, const float* sse) {
  return g && g->flag && __builtin_isfinite(sse[0]) && g->headroom > kHeadroomMin;
}
// a fused last layer's hand-off timed out: the step's loss and gradients are void
__device__ __forceinline__ bool guard_stalled(const GuardState* g) { return g && g->stalls != 0; }
// the update is skipped (Adam leaves p, m, v untouched; the scheduler does not step)
__device__ __forceinline__ bool guard_skip(const GuardState* g, const float* sse) {
  return guard_stalled(g) || guard_overflow(g, sse);
}
// sse (nullable): the reduced [sse, stall slot] pair of siren_grads (a non-zero stall slot marks the guard stalled)
hipError_t guard_check(const float* g, int64_t n, GuardState* guard, hipStream_t s, const float* sse = nullptr);
// a0 / E0 non-null: Linear + Snake first layer (first_linear=True); C0 null: Y0 only
hipError_t first_fwd(const float* t, int in_dim, const float* W0, const float* b0, float omega0,
                     int R, int H, h16* Y0, h16* C0, hipStream_t s, const float* a0 = nullptr,
                     h16* E0 = nullptr);
hipError_t head_loss(const float* head_part, int nparts, int R, const float* b_head, const float* y,
                     int n_valid, float gfac, float* out, float* g, float* sse_part,
                     float* gsum_part, float* gmax_part, hipStream_t s, float head_omega = 0.f,
                     int loss_mode = 0);
hipError_t gmax_partials(const float* g, int R, float* gmax_part, hipStream_t s);
hipError_t head_sine_chain(const float* head_part, int nparts, int R, const float* b_head, float omega, float* g,
                           hipStream_t s);
// S before the forward (NT_FWD_HB): from a loss-independent bound of max|g| -- ymax_part holds
// (n_valid+255)/256 max|target| partials; act_bound = |dY/dz| bound of the last layer
hipError_t grad_scale_bound(const float* ymax_part, int nparts, const float* w_head, const float* b_head, int H,
                            float gfac, float head_omega, int loss_mode, float act_bound, float* gscale,
                            hipStream_t s, const GuardState* guard = nullptr);
// gscale[0] = S (dZ storage scale), gscale[1] = 1/S; from (R+255)/256 max|g| partials
hipError_t grad_scale(const float* gmax_part, int nparts, const float* w_head, int H, float omega,
                      float* gscale, hipStream_t s, const GuardState* guard = nullptr);
// E != null (Snake last layer): da_part[R/128][H] = partial sums of g*w_head*E
hipError_t head_bwd(const h16* C, const h16* Y, const float* g, const float* w_head, float omega,
                    int R, int H, const float* gscale, h16* dZ, float* db_part, float* dwh_part,
                    const h16* E, float* da_part, hipStream_t s);
// out[c*out_stride] (+)= sum_r part[r*row_stride + c]; tmp holds >= 64*ncols floats
hipError_t col_reduce(const float* part, int64_t row_stride, int nrows, int ncols, float* out,
                      int out_stride, int accumulate, float* tmp, hipStream_t s);
// up to kMaxColSegs col_reduce of one partial-row layout in one launch pair (results identical to
// one col_reduce per segment); tmp holds >= n*64*ncols floats
constexpr int kMaxColSegs = 4;
struct ColSegs {
  const float* src[kMaxColSegs];
  float* out[kMaxColSegs];
  int out_stride[kMaxColSegs];
  int n;
};
hipError_t col_reduce_multi(const ColSegs& sg, int64_t row_stride, int nrows, int ncols, int accumulate, float* tmp,
                            hipStream_t s);

// unfused fp32 layers (layer_fp32.hip): lone SineLayer / Linear / Snake / Tanh modules
enum Fp32Act { FP32_IDENTITY = 0, FP32_SIN = 1, FP32_TANH = 2, FP32_SNAKE = 3 };  // == siren_fp32_act
hipError_t fp32_linear(const float* x, int64_t rows, int in, int out, const float* W, const float* b, float omega,
                       float* pre, hipStream_t s);
hipError_t fp32_act(int act, const float* x, int64_t rows, int cols, const float* a, float* y, hipStream_t s);
hipError_t fp32_act_bwd(int act, const float* x, int64_t rows, int cols, const float* a, const float* gy,
                        float* gpre, float* da_prod, hipStream_t s);
hipError_t fp32_linear_bwd(const float* x, int64_t rows, int in, int out, const float* W, float omega, float* gpre,
                           float* gx, float* gW, float* gb, float* slab, int splits, float* tmp, hipStream_t s);

// Gaussian random-Fourier-feature encoded first layer (rff.hip; run.py:141-144): x [R][1], Bf [F],
// enc = [cos(2 pi x Bf) | sin(2 pi x Bf)], W0 [H][2F].  enc buffers are fp16 [R][rff_kpad(F)]
constexpr int kRffMaxFreq = 256;
int rff_kpad(int F);                          // 2F padded to the weight-gradient GEMM's 128-column tile
int rff_splits(int R, int H, int F);          // split-K slices of the dW0 GEMM
int64_t rff_slab_floats(int R, int H, int F);  // [splits + 1][H][kpad] + [H]
hipError_t rff_encode(const float* x, const float* Bf, int F, int64_t rows, float* out, hipStream_t s);
hipError_t rff_encode16(const float* x, const float* Bf, int F, int R, h16* enc, hipStream_t s);
// a0 / E0 non-null: Linear + Snake first layer; enc nullable (inference)
hipError_t rff_first_fwd(const float* x, const float* Bf, int F, const float* W0, const float* b0, float omega0, int R,
                         int H, h16* Y0, h16* C0, const float* a0, h16* E0, h16* enc, hipStream_t s);
// gW0 [H][2F] += scale (dZ0^T enc) / S and (db non-null) gb0 += scale db; slab: rff_slab_floats
hipError_t rff_dw0(const h16* enc, const h16* dZ0, int F, int R, int H, float scale, const float* gscale,
                   float* slab, const float* db, float* gW0, float* gb0, hipStream_t s);

// The spectral losses and the loss mix (stft.hip; run.py:126-128, :160-169): the single STFT loss
// (n_fft / hop / win 1024 / 256 / 1024), the multi-resolution one (1024 / 120 / 600, 2048 / 240 / 1200,
// 512 / 50 / 240; L = (L_0 + L_1 + L_2) / 3) and the SNR loss.  One caller-owned fp32 workspace of
// spec_ws_map's `total` floats per loss, carved up by spec_ws_map
enum SpecLoss { SPEC_STFT = 0, SPEC_MRSTFT = 1 };
// a loss's transforms need n > its largest n_fft / 2 (reflect padding)
constexpr int kStftMinN = 512, kMrRes = 3, kMrMinN = 1024, kMrScalFloats = 32;
struct SpecRes {          // one transform (T frames, bins and window support padded to 16)
  float *re, *im;         // [T][bins] transform of the model output
  float *ymag, *ylog;     // [T][bins] target magnitudes and their logs (constant: spec_forward(target))
  float* dF;              // [T][win] gradient of the frames over the window's support
  float* part;            // rows PT_S1, PT_SL of [.][npart] per-block partial sums
  float* scal;            // its finished scalars SC_S1 .. SC_C2
  int T, npart;
};
struct PointWs {          // the point loss (L1 / MSE / SNR)
  float* part;            // [PT_ROWS][npart] per-block partial sums
  float* scal;            // [32] finished scalars (SC_*)
  float* gchain;          // [rows] dLoss/d(head linear output) of a last_linear=False step
  int npart;
};
// SPEC_STFT: r[0].part / .scal / .npart and scal are pt's (one block of partials, one scal[32]);
// SPEC_MRSTFT: r[i].part is [2][npart_i], r[i].scal = scal + MR_SLOTS i, scal[kMrScalFloats] its own
struct SpecWs {
  SpecLoss loss;
  int nres;               // 1 / kMrRes
  SpecRes r[kMrRes];
  float* scal;
  PointWs pt;
};
// PointWs::scal slots; SC_S1 .. SC_C2 are also the slots of every SpecRes::scal
enum { SC_S1 = 0, SC_SL = 1, SC_SY = 2, SC_LSTFT = 3, SC_C1 = 4, SC_C2 = 5, SC_MX = 6, SC_MY = 7, SC_SYC = 8,
       SC_SR = 9, SC_LSNR = 10, SC_FSNR = 11, SC_LPOINT = 12, SC_LOSS = 13 };
// SPEC_MRSTFT's SpecWs::scal: MR_SLOTS floats per resolution, then the mean, the point loss and the mixed loss
enum { MR_SLOTS = 8, MR_MEAN = 0, MR_POINT = 1, MR_LOSS = 2 };
// part[] rows (each npart floats)
// (the SNR sums are kept as a float pair hi + lo: L_snr crosses zero where the fit's residual
// equals the signal, and an fp32 sum's 2^-24 is 1e-5 of a loss of 0.007 dB)
enum { PT_S1 = 0, PT_SL = 1, PT_SX = 2, PT_SYM = 3, PT_SYC = 4, PT_SR = 5, PT_SYC_LO = 6, PT_SR_LO = 7, PT_ROWS = 8 };
// the split step keeps the L1 / MSE partials per 256 samples of the whole signal in the row
// that only the SNR loss uses otherwise (a one-batch step has them in siren_batch.sse_part)
enum { PT_SSE = PT_SX };
int64_t spec_frames(SpecLoss k, int64_t n, int r);   // 1 + n / hop_r (0: n too short for the loss, or no such r)
int64_t spec_basis_floats(SpecLoss k);
void spec_basis_fill(SpecLoss k, float* host);  // per transform both table layouts, fp64 on the host rounded once
SpecWs spec_ws_map(SpecLoss k, float* ws, int n, int rows, int64_t* total = nullptr);
// frame blocks (16 frames each) of transform r over the whole signal, and its forward grid.y: the block
// (bx, by) writes the partial by * spec_frame_blocks + bx of its two rows
int spec_frame_blocks(SpecLoss k, int64_t n, int r);
int spec_grid_y(SpecLoss k, int r);
// the frame blocks of transform r that the samples [lo, hi) need (compute) and contribute partials for (owned)
void spec_window(SpecLoss k, int r, int n, int lo, int hi, int compute[2], int owned[2]);
// target: ymag, ylog and Sy per transform; else re, im and the partials of S1 and sum|dlog|
// win (model side; null: every block): per transform the frame blocks [win[2 r], win[2 r + 1]) that run
hipError_t spec_forward(const float* x, int n, const float* basis, const SpecWs& w, bool target, hipStream_t s,
                        const int* win = nullptr);
// the L1 (loss_mode 1) / MSE partials per 256 samples of out against y -> row PT_SSE of w.pt.part
hipError_t point_partials(const float* out, const float* y, int n, int loss_mode, const SpecWs& w, hipStream_t s);
// partials of the means, then of sum yc^2 and sum (xc - yc)^2
hipError_t snr_sums(const float* x, const float* y, int n, const SpecWs& w, hipStream_t s);
// the point loss's finished scalars; loss_mode 0 / 1: sum(sse_part) / n_total, 2: L_snr, -1: none.
// stft (SPEC_STFT only): the partials of spec_forward are reduced and loss = (1 - alpha) point +
// alpha L_stft (loss_mode -1: L_stft); loss_out (nullable) <- the loss
hipError_t loss_finish(const SpecWs& w, int n, const float* sse_part, int nsum, int loss_mode, double alpha,
                       double n_total, bool stft, float* loss_out, hipStream_t s);
// SPEC_MRSTFT's finished scalars; stft: the partials of spec_forward are reduced; loss_mode >= 0: the point
// loss is loss_finish's, -1: none (loss = L_mrstft); loss_out[0] (nullable) <- the mixed loss, terms:
// loss_out[1..3] <- L_0, L_1, L_2
hipError_t mrstft_finish(const SpecWs& w, bool stft, int loss_mode, double alpha, float* loss_out, bool terms,
                         hipStream_t s);
hipError_t spec_backward(const float* basis, const SpecWs& w, hipStream_t s, const int* win = nullptr);  // -> r[i].dF
hipError_t spec_gather(int n, const SpecWs& w, float* g, hipStream_t s);        // dF -> dL_stft / dL_mrstft / dx [n]
// g[lo .. rows) = (1 - alpha) g_point + alpha gather(dF), 0 on pad rows
hipError_t loss_mix(const float* out, const float* y, int n, int rows, const SpecWs& w, int loss_mode, double alpha,
                    float gfac, float* g, hipStream_t s, int lo = 0);

// KAN (kan.hip, kan_general.hip): fp32, spline_order 3, any grid size G = 1 .. KG_MAX_GRID:
// NB = G + 3 bases, NG = G + 7 knots, K1 = G + 4 A-columns per input.  grid [in][G + 7],
// spline_w [out][in][G + 3], W [out][(G + 4) in]; slabs of out x (G + 4) in floats.
constexpr int KAN_NB = 8;           // grid_size 5: grid_size + spline_order bases per input
constexpr int KAN_K1 = 1 + KAN_NB;  // A-columns per input feature: SiLU + the bases
constexpr int KG_MAX_GRID = 64;
// A net's grid size and which kernel set runs it (chosen in one place, capi.hip's kan_sel): the
// grid-5 kernels of kan.hip (sizes at compile time, a one-pass hidden backward) or the
// any-grid-size kernels of kan_general.hip (G as a launch argument)
struct KanSel {
  int G, k1;  // k1 = G + 4
  bool general;
};
// capi.hip's per-launch profiling brackets (SIREN_PROF), for kan_hidden_bwd, whose launches fall
// under two kinds (SIREN_PROF_KAN_DW, SIREN_PROF_KAN_DX)
void prof_begin(int kind, hipStream_t s);
void prof_end(hipStream_t s, int launches = 1);
constexpr int KAN_PROF_DW = 9, KAN_PROF_DX = 10;
// fused layer kernels (the bases are recomputed in LDS; A and dA never reach HBM)
hipError_t kan_fwd_fused(const KanSel& k, const float* X, const float* grid, const float* W, int64_t N, int in, int out,
                         float* Y, hipStream_t s);
// split-K over the rows: at most max_splits slabs of out x K1 in floats
hipError_t kan_dw_fused(const KanSel& k, const float* X, const float* grid, const float* G, int64_t N, int in, int out,
                        int64_t max_splits, float* slab, float* dW, hipStream_t s);
hipError_t kan_dx_fused(const KanSel& k, const float* X, const float* grid, const float* Gout, const float* WT,
                        int64_t N, int in, int out, float* Gin, hipStream_t s);
// a hidden layer's backward: dW and (Gin != null) Gin, in one pass where the set has one (grid 5,
// out <= 64: bases and G rows read once), else kan_dw_fused then kan_dx_fused
hipError_t kan_hidden_bwd(const KanSel& k, const float* X, const float* grid, const float* G, const float* WT,
                          int64_t N, int in, int out, int64_t max_splits, float* slab, float* dW, float* Gin,
                          hipStream_t s);
// the last layer (out = 1, in <= 64): wave-per-row forward (inference)
hipError_t kan_head_fwd(const KanSel& k, const float* X, const float* grid, const float* W, int64_t N, int in, float* Y,
                        hipStream_t s);
// the last layer's forward + loss gradient + backward in one pass (out = 1, in <= 64); *nparts
// loss partials (loss_mode 0: MSE, squared errors; 1: L1, absolute errors)
hipError_t kan_head_train(const KanSel& k, const float* X, const float* grid, const float* W, const float* y, int64_t N,
                          int in, int64_t n_valid, float gfac, int64_t slots, int64_t max_parts, float* out, float* g,
                          float* sse_part, float* slab, float* dW, float* Gin, int* nparts, hipStream_t s,
                          int loss_mode = 0);
// its backward half for a given g [N] (zero on pad rows): Gin and dW in kan_head_train's block
// partition and accumulation order for the same slots and max_parts
hipError_t kan_head_bwd(const KanSel& k, const float* X, const float* grid, const float* W, const float* g, int64_t N,
                        int in, int64_t slots, int64_t max_parts, float* slab, float* dW, float* Gin, hipStream_t s);
// W = [base_w | spline_w * scaler] as [out][K1 in], and (WT != null) its transpose [K1 in][out]
hipError_t kan_combine(const KanSel& k, const float* base_w, const float* spline_w, const float* scaler, int out, int in,
                       float* W, float* WT, hipStream_t s);
hipError_t kan_param_grads(const KanSel& k, const float* dW, const float* spline_w, const float* scaler, int out, int in,
                           int accumulate, float* g_base, float* g_spline, float* g_scaler, hipStream_t s);
hipError_t kan_gemm(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, int M,
                    int N, int64_t K, int splits, float* C, float* out, hipStream_t s);
// The refit of update_grid (kan.py:168-215, Go = Gn) and of regrid (kan_general.hip, "the refit"): old
// knots [in][Go + 7], new knots [in][Gn + 7], both sizes 1 .. KG_MAX_GRID.  New knots from the order
// statistics q [Gn + 1][in] (margin2 = fp32(2 margin), one_eps = fp32(1 - grid_eps): the reference's
// host scalars).  gram [in]{G_nn [Gn+3][Gn+3], G_no [Gn+3][Go+3]} (fp64: G_nn = sum b_new b_new^T,
// G_no = sum b_new b_old^T over the N rows of X), added to gram's contents when `accumulate`; part:
// kan_regrid_part_doubles doubles of scratch (what can be non-zero; the dense pair at 5 -> 5);
// pass_rows: the rows one pass of the Gram kernel's grid covers.  spline_w_new = fp32(G_nn^-1 G_no
// (spline_w * scaler)) per input, scaler may be null (all ones), no scratch; status[0] = rank-deficient
// inputs (pivot <= 2^-40 max diagonal), status[1] = the first of them
hipError_t kan_regrid_knots(const float* q, int in, int Gn, float margin, float margin2, float eps, float one_eps,
                            float* grid, hipStream_t s);
int kan_regrid_slices(int64_t N, int in, int Go, int Gn);
int64_t kan_regrid_pass_rows(int in, int Go, int Gn);
int64_t kan_regrid_part_doubles(int64_t N, int in, int Go, int Gn);
hipError_t kan_regrid_gram(const float* X, const float* grid_old, const float* grid_new, int64_t N, int in, int Go,
                           int Gn, int accumulate, double* part, double* gram, hipStream_t s);
hipError_t kan_regrid_refit(const double* gram, int in, int out, int Go, int Gn, const float* spline_w,
                            const float* scaler, float* spline_w_new, int* status, hipStream_t s);

struct OptState {      // device-resident optimizer + ReduceLROnPlateau state (run.py:116-117)
  double lr;           // current learning rate (param_groups[0]['lr'])
  double best;         // plateau: best loss so far (init +inf)
  double step;         // Adam step count (torch keeps it as a float tensor)
  int32_t num_bad;     // plateau: num_bad_epochs
  int32_t last_epoch;  // number of scheduler.step() calls
  double min_lr, factor, threshold, eps_lr;
  int32_t patience, pad0;
  double beta1, beta2, eps;
};

hipError_t adam_flat(float* p, const float* g, float* m, float* v, int64_t n, const OptState* st,
                     hipStream_t s, const GuardState* guard = nullptr, const float* sse = nullptr);
hipError_t plateau_step(OptState* st, const float* sse, double n_total, float* loss_hist,
                        double* lr_hist, int64_t hist_cap, hipStream_t s, GuardState* guard = nullptr);
// The best step so far (include/siren_hip.h siren_best_keep: a plain int32[4], no ABI struct)
struct BestState {
  int32_t loss_bits;  // float bits of the best loss (+inf initially)
  int32_t step;       // its index in loss_hist (-1: none)
  int32_t taken;      // snapshots taken
  int32_t pad;
};
constexpr int kBestKeepGridCap = 2048;  // blocks of 256 threads x one float4: 2 M floats per pass
// best_params[0..n) = params[0..n) (n % 4 == 0, 16-B aligned) and best = {loss, st->last_epoch, ++taken}
// iff this step's loss < best's, sse[1] == 0 and the guard (nullable) is not stalled; two launches
hipError_t best_keep(const float* params, float* best_params, int64_t n, const OptState* st, const float* sse,
                     double n_total, const GuardState* guard, BestState* best, hipStream_t s);
hipError_t cast_weight(const float* W, int H_out, int H_in, h16* Wb, h16* WTb, hipStream_t s);
// cast_weight of n square H x H layers in one launch
constexpr int kMaxInner = 16;  // == SIREN_MAX_INNER
struct CastSet {
  const float* W[kMaxInner];
  h16* Wb[kMaxInner];
  h16* WTb[kMaxInner];
  int n;
};
hipError_t cast_weights(const CastSet& cs, int H, hipStream_t s);

// The loss-landscape plane (plane.hip; run.py:192-198): one grid point's parameters and shadows.
// A flat fp32 parameter vector of n4 float4 holds n square H x H hidden weights at float offsets
// w_off[l]; [lo[r], hi[r]) (float4 units, nrest of them) are the pieces of the vector outside them
struct PlaneSet {
  int64_t w_off[kMaxInner];
  h16* Wb[kMaxInner];
  h16* WTb[kMaxInner];
  int64_t lo[kMaxInner + 1], hi[kMaxInner + 1];
  int n, nrest;
};
// out = fma(b, d2, fma(a, d1, theta)) over the whole vector; Wb / WTb = cast_weight of out's hidden weights
hipError_t plane_point(const float* theta, const float* d1, const float* d2, float a, float b, float* out,
                       const PlaneSet& ps, int H, hipStream_t s);
// slot[0] += sum of sse_part[0 .. nparts) in fp64, in a fixed order
hipError_t plane_loss(const float* sse_part, int nparts, double* slot, hipStream_t s);
hipError_t sum_to(const float* x, int n, float* out, int accumulate, hipStream_t s);
// sum_to(x0 -> out0) and sum_to(x1 -> out1) in one launch; flag_src non-null: also
// flag_dst[0] (+)= (flag_src[0] != 0)
hipError_t sum_to2(const float* x0, float* out0, const float* x1, float* out1, int n, int accumulate, hipStream_t s,
                   const int* flag_src = nullptr, float* flag_dst = nullptr);

}  // namespace siren
