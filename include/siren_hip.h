/*
 * siren_hip.h -- C-ABI of libsiren_hip.so, the MI355X (gfx950) SIREN audio-fitting path.
 *
 * The reference (senyuanfan/inr-for-audio) is pure PyTorch and has no FFI; each entry point
 * below replaces the torch eager work behind one reference interface, cited as file:line
 * into the reference tree.  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (torch allocates; the library
 *     never allocates, frees or synchronises the host);
 *   - 16-bit tensors (activations, cosines, weight shadows, pre-activation gradients) are
 *     IEEE fp16 passed as uint16_t*, row-major (DESIGN.md "Storage precision": fp16 keeps
 *     the fit at the fp32 reference's quality where bf16 costs ~1.3 dB); fp32 weights use
 *     the nn.Linear layout [out_features][in_features];
 *   - backward pre-activation gradients dZ are stored multiplied by a power-of-two scale
 *     S = gscale[0] (siren_grad_scale); every fp32 gradient leaves unscaled;
 *   - `stream` is a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream);
 *   - every function returns 0 on success, or a non-zero siren_status / hipError_t code
 *     (see siren_status_string), and never aborts the process.
 */
#ifndef SIREN_HIP_H
#define SIREN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIREN_ABI_VERSION 12
#define SIREN_MAX_INNER 16  /* max hidden layers (num_sine + num_snake + num_tanh) */
/* hidden widths: 128, 256, 512, 1024, then multiples of 1024 up to this (run as 1024-column
 * windows; models.py pads any other width to the next of these) */
#define SIREN_MAX_HIDDEN 4096
#define SIREN_ROW_TILE 128  /* coordinate rows are padded to a multiple of this */
/* ints in one tile-queue counter set (siren_batch.tileq, siren_inner_fwd's tileq): the
 * hidden-layer forward GEMM's persistent blocks pull their tiles from it.  Caller-owned device
 * memory, any content: the library zeroes it on the stream before every launch that uses it.
 * One set serves every launch of one stream in order; launches that may run concurrently
 * (other streams, other devices, replays of other captured graphs) need sets of their own. */
#define SIREN_TILEQ_INTS 768

enum siren_status {
  SIREN_OK = 0,
  SIREN_ERR_SHAPE = 1001,   /* unsupported / inconsistent shape            */
  SIREN_ERR_NULL = 1002,    /* required pointer missing                    */
  SIREN_ERR_CONFIG = 1003   /* unsupported configuration (e.g. in_dim > 2) */
};

int siren_abi_version(void);
/* ABI 12: hex SHA-256 of the sources this library was compiled from (the .hip and .h files of csrc and this
 * header) and of its compile defines -- the binding compares it with the sources beside it, so a
 * stale or foreign library is refused instead of trusted by file time */
const char* siren_build_id(void);
/* sizeof of the ABI structs, for binding checks: 0 siren_net, 1 siren_grads, 2 siren_batch,
 * 3 siren_opt_state, 4 siren_kan_net, 5 siren_kan_grads, 6 siren_kan_batch, 7 siren_guard,
 * 8 siren_spectral, 9 siren_spectral_mr (-1: unknown) */
int64_t siren_struct_size(int32_t which);
const char* siren_status_string(int status);

/* ---- device-resident optimizer state: torch.optim.Adam + ReduceLROnPlateau ------------
 * run.py:116-117 (Adam(lr), ReduceLROnPlateau(mode='min', factor=0.8, patience=200,
 * min_lr=min_learning_rate)).  Layout shared with the Python mirror. */
typedef struct siren_opt_state {
  double lr, best, step;
  int32_t num_bad, last_epoch;
  double min_lr, factor, threshold, eps_lr;
  int32_t patience, pad0;
  double beta1, beta2, eps;
} siren_opt_state;

/* ---- fp16 backward range guard (device-resident, optional) ---------------------------
 * The backward stores dZ in fp16 times a power-of-two scale S (siren_grad_scale) chosen so
 * that the head's bound lands under 2^headroom.  siren_apply_update checks the reduced fp32
 * gradients: if any is non-finite while the loss is finite (an fp16 overflow of dZ*S, which
 * fp32 autograd in the reference never has), the Adam and scheduler updates are SKIPPED
 * (nothing advances: no step, no history entry), headroom drops by 4, and the caller's next
 * step recomputes the same gradients with a 16x smaller S -- GradScaler-style, but with no
 * optimizer step lost.  After 1000 clean steps headroom grows back by 1 (up to its initial
 * value).  Zero-initialise it and set headroom = 6 (the fixed value used when NULL).
 * ABI 12: `stalls` counts hand-off waits of the fused last layer (siren_train_step with
 * SIREN_OPT_HEAD_FUSE) that gave up because a band partner never published its head partial (a
 * partner kept off the chip, e.g. CUs held by another process).  Such a step's loss and gradients
 * are void: while stalls != 0 siren_apply_update skips Adam and the scheduler (no step, no history
 * entry, headroom untouched) -- the counter is sticky, the caller reads it, reports the failure and
 * zeroes it before training on. */
typedef struct siren_guard {
  int32_t flag;        /* this step: non-finite gradients seen (written by apply_update)  */
  int32_t headroom;    /* S exponent target: max|g| max|w_head| omega S < 2^headroom       */
  int32_t clean;       /* consecutive clean steps since the last overflow                   */
  int32_t overflows;   /* steps skipped and recomputed so far                               */
  int32_t headroom0;   /* initial / maximum headroom                                       */
  int32_t stalls;      /* fused last layer: timed-out hand-off waits (sticky; ABI 12)       */
} siren_guard;

/* ---- one L x H network (SirenWithSnakeTanh, models.py:306-394) ------------------------
 * net.0 = SineLayer(in, H, is_first, omega0); then L inner layers H -> H, each a
 * SineLayer(H, H, omega) (models.py:114-115), a Linear + Snake(a) (models.py:356-364,
 * 235-241) or a Linear + Tanh (models.py:366-372), in the reference's order (num_sine
 * sines, then num_snake Snakes, then num_tanh Tanhs); last: Linear(H, 1).  act[i] says
 * which (siren_act); a[i] is the Snake's per-channel a [H]. */
enum siren_act { SIREN_ACT_SINE = 0, SIREN_ACT_SNAKE = 1, SIREN_ACT_TANH = 2 };
typedef struct siren_net {
  int32_t in_dim, hidden, n_inner, pad0;
  float omega0, omega;
  const float* W0;                          /* [H][in]  fp32 */
  const float* b0;                          /* [H]           */
  const float* b[SIREN_MAX_INNER];          /* [H]           */
  const uint16_t* Wh[SIREN_MAX_INNER];      /* [H][H] fp16 shadow of W_i   */
  const uint16_t* WTh[SIREN_MAX_INNER];     /* [H][H] fp16 shadow of W_i^T */
  const float* w_head;                      /* [H] (last Linear's weight[0]) */
  const float* b_head;                      /* [1]                          */
  int32_t act[SIREN_MAX_INNER];             /* siren_act of inner layer i   */
  const float* a[SIREN_MAX_INNER];          /* [H] Snake a (SNAKE layers)   */
  /* first_linear=True (models.py:330-333): net.0 is Linear(in, H) + Snake(a0) instead of the
   * first SineLayer (omega0 unused); last_linear=False (models.py:383-385): the last layer is
   * SineLayer(H, 1, head_omega) -- out = sin(head_omega (Y w^T + b)); 0 = the final Linear */
  int32_t first_snake, pad1;
  const float* a0;                          /* [H] (first_snake)            */
  float head_omega, pad2;
  /* run.py:141-144 rff.layers.GaussianEncoding(sigma, 1, rff_freq) in front of net.0 (appended in
   * ABI 12; 0 = none): coords stay the raw [rows][1] coordinate (in_dim must be 1), rff_B is the
   * encoding's b [rff_freq][1] fp32 (not trained) and W0 is [H][2 rff_freq] -- net.0 sees
   * cat(cos(2 pi x b^T), sin(2 pi x b^T)), built inside the first layer's kernel.  1..256. */
  int32_t rff_freq, pad3;
  const float* rff_B;
} siren_net;

/* gradient destinations (fp32, accumulated into: zero them, or set zero_grads) */
typedef struct siren_grads {
  float* W0; float* b0;
  float* W[SIREN_MAX_INNER]; float* b[SIREN_MAX_INNER];
  float* w_head; float* b_head;
  float* sse;                               /* [2] sum of squared errors of valid rows, then (ABI 12)
                                               the fused hand-off's stall flag: both accumulate like the
                                               gradients and ride the same all-reduce */
  float* flat; int64_t flat_len;            /* if flat != NULL and zero_grads: memset   */
  float* a[SIREN_MAX_INNER];                /* [H] Snake a gradients (SNAKE layers)     */
  float* a0;                                /* [H] first-layer Snake a (first_snake)    */
} siren_grads;

/* per-micro-batch activations and workspace; sizes from siren_workspace_floats() */
typedef struct siren_batch {
  int32_t rows;          /* padded rows, multiple of SIREN_ROW_TILE          */
  int32_t n_valid;       /* valid rows (<= rows)                             */
  double n_total;        /* global coordinate count: MSE mean denominator    */
  int32_t splits;        /* split-K slices of the weight-gradient GEMM       */
  int32_t zero_grads;    /* 1: zero `grads.flat` before accumulating         */
  const float* coords;   /* [rows][in]  (net.rff_freq > 0: the raw [rows][1] coordinate) */
  const float* target;   /* [rows]      */
  uint16_t* Y[SIREN_MAX_INNER + 1];  /* Y[0..L] fp16 [rows][H]: layer outputs          */
  uint16_t* C[SIREN_MAX_INNER + 1];  /* C[0..L] fp16 [rows][H]: cos(.) of a sine layer,
                                        dY/dz of a Snake / Tanh layer                 */
  uint16_t* dZ[2];       /* fp16 [rows][H] ping-pong pre-activation gradients x S */
  float* out;            /* [rows] model output                                 */
  float* g;              /* [rows] dLoss/dout                                   */
  float* head_part;      /* [H/128][rows]                                       */
  float* sse_part;       /* [rows/256]                                          */
  float* gsum_part;      /* [rows/256]                                          */
  float* gmax_part;      /* [rows/256]  max |g| per block (train / backward)    */
  float* gscale;         /* [2]  {S, 1/S} of this micro-batch's backward        */
  float* col_part;       /* [rows/128][max(2, 2+in)][H]                         */
  float* col_part2;      /* [rows/128][H]                                       */
  float* red_tmp;        /* [4][64][H]  (ABI 10; was [64][H])                   */
  float* slab;           /* [splits][H][H]                                      */
  uint16_t* E[SIREN_MAX_INNER + 1];  /* E[i+1] fp16 [rows][H]: dY/da of Snake inner layer
                                        i; E[0]: of a Linear + Snake first layer (NULL
                                        for other layers)                              */
  /* optional gradient-ready events (hipEvent_t, NULL = none), recorded on `stream` as soon
   * as a bucket's gradients are final in this call -- set them on the LAST micro-batch so a
   * data-parallel caller can all-reduce each bucket on a communication stream while the rest
   * of the backward runs.  [i < L]: inner layer i (W_i, b_i, Snake a_i);
   * [L]: the first layer (W0, b0); [L+1]: the head (w_head, b_head) and `sse`. */
  void* grad_ready[SIREN_MAX_INNER + 2];
  /* run.py:161-169 loss_mode: 0 = MSELoss (sse = sum err^2, g = 2 err / n_total), 1 = L1Loss
   * ('mae': sse slot = sum |err|, g = sign(err) / n_total), 2 = the SNR loss ('snr', run.py:126,
   * :165): siren_train_step_spectral only (siren_train_step has no workspace for it: SIREN_ERR_NULL) */
  int32_t loss_mode;
  /* ABI 11: 1 = gmax_part holds the max|g| partials of a previous siren_train_step /
   * siren_backward on this workspace (same rows).  A Snake last layer then runs fused with the
   * head (the backward scale S must be fixed before the forward, and |Y_L| has no bound, so S is
   * taken from those partials; the range guard catches a step whose |g| outgrew it).  0: a Snake
   * last layer runs unfused.  Sine / Tanh last layers ignore it. */
  int32_t head_scale_prev;
  /* range guard (NULL: fixed headroom 6, no overflow recovery, and the last layer runs unfused).
   * ABI 12: not const -- a fused last layer whose hand-off wait times out counts it in
   * guard->stalls, which voids the step */
  siren_guard* guard;
  int32_t* tileq;            /* SIREN_TILEQ_INTS ints of tile-queue counters on the device of the
                                activations (NULL: the forward GEMM's static tile walk) */
  /* net.rff_freq > 0 (appended in ABI 12): enc = fp16 [rows][siren_rff_kpad(rff_freq)], the
   * encoded coordinates the first layer's forward writes once for its weight gradient (NULL at
   * inference: not written); rff_slab = siren_rff_slab_floats(rows, hidden, rff_freq) floats, the
   * encoded layer's own split-K slab (train / backward) */
  uint16_t* enc;
  float* rff_slab;
} siren_batch;

/* Workspace sizing / tiling helpers.  siren_nt_tile: tile edge the NT GEMMs use for
 * `rows` coordinates (partial-sum buffers then hold rows/tile rows and head partials
 * hidden/tile rows); siren_dw_tile: tile edge of the weight-gradient GEMM. */
int32_t siren_nt_tile(int32_t rows, int32_t hidden);
int32_t siren_dw_tile(int32_t rows, int32_t hidden);
int32_t siren_default_splits(int32_t rows, int32_t hidden);
int64_t siren_slab_floats(int32_t hidden, int32_t splits);

/* ---- fused path ---------------------------------------------------------------------
 * siren_forward:     run.py:158 / :255  model(model_input) -> batch.out (inference only).
 * siren_train_step:  run.py:158-185     forward + MSELoss + loss.backward() for one
 *                    micro-batch; gradients ACCUMULATE into `grads` (global-N scaling).
 * siren_apply_update:run.py:186-187     optimizer.step() + scheduler.step(loss), then the
 *                    fp16 weight shadows are refreshed.  (`params`, `grads_flat`, `exp_avg`,
 *                    `exp_avg_sq` are the flat fp32 vectors of length n_params.)          */
int siren_forward(const siren_net* net, siren_batch* batch, void* stream);
int siren_train_step(const siren_net* net, const siren_grads* grads, siren_batch* batch,
                     void* stream);
/* loss.backward() through the network for an arbitrary upstream gradient: batch->g holds
 * dLoss/dout (zero on pad rows) and batch->Y/C the activations of a prior siren_forward. */
int siren_backward(const siren_net* net, const siren_grads* grads, siren_batch* batch,
                   void* stream);
int siren_apply_update(const siren_net* net, float* params, const float* grads_flat,
                       float* exp_avg, float* exp_avg_sq, int64_t n_params,
                       float* const* W_fp32 /* [n_inner] views into params */,
                       uint16_t* const* Wh, uint16_t* const* WTh,
                       siren_opt_state* state, const float* sse, double n_total,
                       float* loss_hist, double* lr_hist, int64_t hist_cap,
                       siren_guard* guard /* NULL: no range check */, void* stream);
/* (siren_apply_update: `sse` is siren_grads.sse after any all-reduce -- sse[1] != 0 marks the guard
 * stalled, so every rank skips a step any rank's fused hand-off voided) */

/* run.py:171-174 as the reference meant it: the weights of the best step so far.
 * best: int32[4] = {float bits of best loss (+inf initially), best step (-1), snapshots taken, 0}
 * Called on the step's stream BEFORE siren_apply_update / siren_adam_step (and after any all-reduce),
 * while `params` still are the weights the loss in `sse` was computed with.  Two launches, no host
 * synchronisation, capturable in a graph: a float4 copy best_params[0..n) = params[0..n), then one
 * thread that sets best = {loss, state->last_epoch, taken + 1}; both iff
 *   loss = (float)((double)sse[0] / n_total)  (the float siren_plateau_step records at
 *          loss_hist[state->last_epoch])  <  the best loss     -- strict: NaN never wins, a tie keeps
 *                                                                 the earlier step
 *   and sse[1] == 0 and (guard given) guard->stalls == 0       -- a voided step has no loss.
 * The guard's overflow flag is not consulted: the loss of a step whose fp16 backward overflowed is
 * still the true loss of `params`, nothing advances on it, and the recomputed step (same loss, same
 * last_epoch) is not taken again.  n: floats, n >= 4, n % 4 == 0, both vectors 16-B aligned (else
 * SIREN_ERR_SHAPE); n_total > 0 and best_params != params (else SIREN_ERR_CONFIG); NULL params,
 * best_params, state, sse or best: SIREN_ERR_NULL -- all before any launch. */
int siren_best_keep(const float* params, float* best_params, int64_t n,
                    const siren_opt_state* state, const float* sse, double n_total,
                    const siren_guard* guard /* NULL ok */, int32_t* best, void* stream);

/* ---- the loss-landscape plane ---------------------------------------------------------
 * run.py:192-198 (visualization=True): the MSE at steps x steps weight settings
 * theta_ij = theta + a_i d1 + b_j d2 around the fitted weights.
 * siren_plane_point: run.py:192-198  one grid point's weights, one launch.  `theta`, `d1`, `d2` and
 *   `out` are flat fp32 vectors of n_flat floats (n_flat % 4 == 0, 16-B aligned, out != theta) in one
 *   layout; out = fma(b, d2, fma(a, d1, theta)) element by element (fp32, two roundings).  W_out
 *   [n_inner] are the square hidden weights' positions inside `out` (as siren_apply_update's W_fp32
 *   are inside params; float offsets % 4 == 0, no overlap); Wh / WTh receive their fp16 shadows, bit
 *   for bit siren_cast_weight of the fp32 values written to `out`.  Directions are zero in pad entries
 *   and alignment gaps, which therefore keep theta's value.
 * siren_plane_eval:  run.py:192-198  (the metric is run.py:195's MSELoss whatever the fit's loss_mode)
 *   siren_forward's launches on `batch`, the squared error of batch->out against batch->target over
 *   the first n_valid rows, and sse_slot[0] += that sum (fp64, the 256-row partials added in a fixed
 *   order; the caller zeroes the slot and divides by N).  Of the batch it writes the activations, out,
 *   g, head_part, sse_part and gsum_part -- nothing a later training step reads before writing it: not
 *   gmax_part, not siren_grads, not the guard. */
int siren_plane_point(const float* theta, const float* d1, const float* d2, float a, float b, float* out,
                      int64_t n_flat, int32_t hidden, int32_t n_inner,
                      float* const* W_out /* [n_inner] views into out */,
                      uint16_t* const* Wh, uint16_t* const* WTh, void* stream);
int siren_plane_eval(const siren_net* net, siren_batch* batch, double* sse_slot, void* stream);

/* ---- individual kernels (parity tests call these one by one) ------------------------ */
/* utils.py:99-109 get_coord: torch.linspace(-1,1,n_total) at [offset, offset+rows) */
int siren_coords_fill(float* t, int64_t rows, int64_t offset, int64_t n_total, void* stream);
/* utils.py:211-220 MultiWaveformFitting grid, rows [offset, offset+rows) of the height-major
 * (time, channel) grid: xy[r] = (linspace(-1,1,height)[k / width], ch[k % width]) with
 * k = offset + r, ch = linspace(-1,1,width) (all 0 when width == 1); rows past
 * height*width are (0, 0).  Bit-exact with torch.linspace. */
int siren_coords_fill_grid(float* xy, int64_t rows, int64_t offset, int64_t height, int32_t width,
                           void* stream);
/* models.py:114-115 first SineLayer: a0 = omega0*(t W0^T + b0) in fp32, Y0 = sin a0 and
 * C0 = cos a0 (one fp32 sincosf range reduction) -> fp16 */
int siren_first_fwd(const float* t, int32_t in_dim, const float* W0, const float* b0, float omega0,
                    int32_t rows, int32_t hidden, uint16_t* Y0, uint16_t* C0, void* stream);
/* models.py:114-115 hidden SineLayer: Y = sin(omega(X W^T + b)), C = cos(.); optional head
 * partial dot (models.py:374-381) when head_w != NULL; tileq: SIREN_TILEQ_INTS ints for the
 * dynamic tile queue (NULL: static tile walk; results are identical) */
int siren_inner_fwd(const uint16_t* X, const uint16_t* Wh, const float* b, float omega, int32_t rows,
                    int32_t hidden, uint16_t* Y, uint16_t* C, const float* head_w, float* head_part,
                    int32_t* tileq, void* stream);
/* siren_train_step's fused last layer (SIREN_OPT_HEAD_FUSE): models.py:114-115 hidden SineLayer,
 * the head (models.py:374-381), MSELoss / L1Loss gradient (run.py:161-169, loss_mode as
 * siren_batch) and the head backward in one launch -- out, g = dLoss/d(head linear output),
 * 256-row sse / gsum partials (as siren_head_loss), dZ = dZ_L x gscale[0] (as siren_head_bwd) and
 * part[rows/256][2][hidden] = column partials of db_L and dw_head.  Y / C are not written.  Needs
 * rows % 256 == 0 and the 256x256 ping-pong NT tiles (else SIREN_ERR_CONFIG); head_part is
 * [hidden/256][rows] scratch. */
int siren_head_fused_fwd(const uint16_t* X, const uint16_t* Wh, const float* b, float omega, int32_t rows,
                         int32_t hidden, const float* w_head, const float* b_head, float head_omega, const float* y,
                         int32_t n_valid, double n_total, int32_t loss_mode, const float* gscale, float* head_part,
                         float* out, float* g, float* sse_part, float* gsum_part, uint16_t* dZ, float* part,
                         void* stream);
/* ABI 11: siren_head_fused_fwd for a last inner layer of any kind (act, siren_act): SINE as
 * siren_head_fused_fwd; SNAKE (models.py:235-241, a = its [hidden] a) and TANH (models.py:366-372)
 * with their derivative in place of the cosine (omega unused) -- dZ, out, g and the partials as
 * siren_inner_fwd_act -> siren_head_loss -> siren_head_bwd compute them at the same gscale;
 * part[rows/256][2][hidden] (db_L, dw_head), Snake part[rows/256][3][hidden] (+ da_L);
 * gmax_part (nullable): [rows/256] max|g| per 256 rows, as siren_head_loss writes it; E (Snake,
 * else ignored): fp16 [rows][hidden], receives the layer's dY/da as siren_inner_fwd_act writes it
 * (the kernel reads it back for the da_L partials) */
int siren_head_fused_fwd_act(const uint16_t* X, const uint16_t* Wh, const float* b, int32_t act, float omega,
                             const float* a, int32_t rows, int32_t hidden, const float* w_head, const float* b_head,
                             float head_omega, const float* y, int32_t n_valid, double n_total, int32_t loss_mode,
                             const float* gscale, float* head_part, float* out, float* g, float* sse_part,
                             float* gsum_part, float* gmax_part, uint16_t* dZ, float* part, uint16_t* E,
                             void* stream);
/* the fused head's backward scale, fixed before the forward: gscale = {S, 1/S} from a bound of
 * max|g| (MSE: (sum|w_head| + |b_head| + max|y|) 2/n_total, or 1 + max|y| through a final sine of
 * head_omega; L1: 1/n_total; x head_omega) x max|w_head| x act_bound (|dY/dz| bound of the last
 * layer); max|y| over the n_valid target rows, ymax_part = (n_valid+255)/256 floats of scratch */
int siren_grad_scale_bound(const float* y, int32_t n_valid, float* ymax_part, const float* w_head,
                           const float* b_head, int32_t hidden, double n_total, float head_omega, int32_t loss_mode,
                           float act_bound, float* gscale, void* stream);
/* any inner layer kind: SINE as siren_inner_fwd; SNAKE (models.py:235-241): z = X W^T + b,
 * Y = z + sin^2(a z)/a, C = 1 + sin(2az), E = (z sin(2az) - sin^2(az)/a)/a; TANH
 * (models.py:366-372): Y = tanh z, C = 1 - Y^2 (a, E unused) */
int siren_inner_fwd_act(const uint16_t* X, const uint16_t* Wh, const float* b, int32_t act,
                        float omega, const float* a, int32_t rows, int32_t hidden, uint16_t* Y,
                        uint16_t* C, uint16_t* E, const float* head_w, float* head_part,
                        int32_t* tileq, void* stream);
/* run.py:125,168 MSELoss + final Linear bias: out, g = 2(out-y)/n_total, partial sums
 * (gmax_part may be NULL); the L1Loss of loss_mode 1 is reached through siren_train_step */
int siren_head_loss(const float* head_part, int32_t nparts, int32_t rows, const float* b_head,
                    const float* y, int32_t n_valid, double n_total, float* out, float* g,
                    float* sse_part, float* gsum_part, float* gmax_part, void* stream);
/* backward storage scale: gscale = {S, 1/S}, S = 2^k with max|g|*max|w_head|*omega*S < 2^6,
 * from the nparts = rows/256 max |g| partials of siren_head_loss (siren_train_step takes the
 * exponent from batch->guard->headroom instead of 6) */
int siren_grad_scale(const float* gmax_part, int32_t nparts, const float* w_head, int32_t hidden,
                     float omega, float* gscale, void* stream);
/* autograd of Linear(H,1) + the last layer's activation: dZ_L = g w_head omega C (x S),
 * db_L partials, dw_head partials (unscaled); gscale NULL = S 1.  Snake / Tanh last layer:
 * omega = 1 (C is their derivative); Snake also passes E and gets da_part (else NULL) */
int siren_head_bwd(const uint16_t* C, const uint16_t* Y, const float* g, const float* w_head,
                   float omega, int32_t rows, int32_t hidden, const float* gscale, uint16_t* dZ,
                   float* db_part, float* dwh_part, const uint16_t* E, float* da_part, void* stream);
/* autograd addmm dX + sin/omega backward of the layer below: dZprev = omega*cos*(dZ W)
 * (carries dZ's scale); db partials multiplied by 1/S (gscale NULL = unscaled) */
int siren_inner_bwd_dx(const uint16_t* dZ, const uint16_t* WTh, const uint16_t* Cprev, float omega_prev,
                       int32_t rows, int32_t hidden, const float* gscale, uint16_t* dZprev,
                       float* db_part, void* stream);
/* the same into a layer below of any kind (act_prev): SINE as above; TANH: dZprev = C (dZ W);
 * SNAKE: dZprev = D (dZ W) and part [rows/tile][2][H] = partials of db and of da = sum (dZ W) E
 * (x 1/S) */
int siren_inner_bwd_dx_act(const uint16_t* dZ, const uint16_t* WTh, const uint16_t* Cprev,
                           const uint16_t* Eprev, int32_t act_prev, float omega_prev, int32_t rows,
                           int32_t hidden, const float* gscale, uint16_t* dZprev, float* part,
                           void* stream);
/* same into the fp32 first layer (C0 from siren_first_fwd): partials [rows/128][1+in][H]
 * of dZ0 and dZ0*t_j (x 1/S); dZ0 itself is never stored */
int siren_first_bwd_dx(const uint16_t* dZ1, const uint16_t* WTh1, const uint16_t* C0, const float* t,
                       int32_t in_dim, float omega0, int32_t rows, int32_t hidden, const float* gscale,
                       float* part, void* stream);
/* ---- Gaussian random-Fourier-feature encoding (run.py:141-144) --------------------------
 * rff.layers.GaussianEncoding(sigma, input_size=1, encoded_size=F): b = randn(F, 1) * sigma,
 * v -> cat(cos(2 pi v b^T), sin(2 pi v b^T), dim=-1), cosines first.  x [rows][1], B = b [F] fp32,
 * F = rff_freq in 1..256 (else SIREN_ERR_CONFIG).  The phase x b is reduced exactly in
 * revolutions in fp32 before the hardware cos / sin. */
/* width of the fp16 enc buffers: 2 rff_freq padded to a multiple of 128 (0: rff_freq out of range) */
int32_t siren_rff_kpad(int32_t rff_freq);
/* floats of siren_batch.rff_slab / siren_rff_first_bwd's slab (0: unsupported shape) */
int64_t siren_rff_slab_floats(int32_t rows, int32_t hidden, int32_t rff_freq);
/* run.py:141-144 encoding(model_input): out = fp32 [rows][2 rff_freq] (the module API) */
int siren_rff_encode(const float* x, const float* B, int32_t rff_freq, int64_t rows, float* out, void* stream);
/* run.py:141-144 + models.py:114-115: the first SineLayer on the encoded coordinate in one launch --
 * a0 = omega0 (enc(x) W0^T + b0) as an exact fp32 product (W0 [hidden][2 rff_freq]), Y0 = sin a0,
 * C0 = cos a0 -> fp16; a != NULL: Linear + Snake(a) instead (first_linear=True, models.py:330-333,
 * E0 required, omega0 unused); enc (nullable): receives enc(x) as fp16 [rows][siren_rff_kpad] */
int siren_rff_first_fwd(const float* x, const float* B, int32_t rff_freq, const float* W0, const float* b0,
                        float omega0, const float* a, int32_t rows, int32_t hidden, uint16_t* Y0, uint16_t* C0,
                        uint16_t* E0, uint16_t* enc, void* stream);
/* autograd of run.py:141-144's encoded first layer given the layer above: dZ0/omega0 = C0 (dZ1 W1)
 * (x S, fp16, written to dZ0 [rows][hidden]; omega0 is applied in fp32 afterwards, it would
 * overflow fp16), gW0 [hidden][2 rff_freq] += omega0 dZ0^T enc(x) / S split-K over the rows, gb0 +=
 * omega0 colsum(dZ0) / S.  E0 != NULL: Linear + Snake first layer (C0 = dY/dz, omega0 unused,
 * ga0 += colsum((dZ1 W1) E0) / S).  enc: fp16 [rows][siren_rff_kpad] scratch (computed here from
 * x and B); part: [rows/128][2][hidden], red_tmp: [4][64][hidden], slab: siren_rff_slab_floats.
 * Rows whose dZ1 is zero (pad rows: g = 0) contribute exactly nothing. */
int siren_rff_first_bwd(const uint16_t* dZ1, const uint16_t* WTh1, const uint16_t* C0, const uint16_t* E0,
                        const float* x, const float* B, int32_t rff_freq, float omega0, int32_t rows,
                        int32_t hidden, const float* gscale, uint16_t* dZ0, uint16_t* enc, float* part,
                        float* red_tmp, float* slab, float* gW0, float* gb0, float* ga0, void* stream);
/* ---- STFT and SNR losses (run.py:126-128 auraloss.freq.STFTLoss() / auraloss.time.SNRLoss(),
 * evaluated at run.py:160-169) ------------------------------------------------------------------
 * Restated from the published auraloss 0.4.0 defaults; x = model output, y = target, both one
 * sequence of n samples:
 *   X = stft(x, n_fft 1024, hop 256, periodic Hann, center, reflect): T = 1 + n / 256 frames, 513 bins
 *   x_mag = sqrt(max(re^2 + im^2, 1e-8));  L_stft = |y_mag - x_mag|_F / |y_mag|_F + mean|log x_mag - log y_mag|
 *   L_snr = -10 log10(sum yc^2 / (sum (xc - yc)^2 + 1e-8) + 1e-8), xc / yc = x / y minus their means
 * The transform is an exact-fp32 MFMA GEMM against windowed cos / -sin tables.  `basis` holds two
 * fragment-native copies of the table v[c][k][bin] (c 0: w_k cos(2 pi k bin / 1024), 1: -w_k sin(.);
 * bin < 528, zero past 512): floats [0, 2*1024*528) as [c][k / 16][bin][k % 16], then the same
 * number as [c][bin / 16][k][bin % 16].  `ws` is one fp32 workspace; siren_stft_ws_offset locates
 * its pieces.  n > 512 (reflect padding is undefined below; else SIREN_ERR_SHAPE), n <= 2^30. */
/* run.py:160 frames of an n-sample signal (0: n <= 512) */
int64_t siren_stft_frames(int64_t n);
int64_t siren_stft_basis_floats(void);
/* run.py:128 the transform's tables, computed in fp64 and rounded once -- `basis_host` is a HOST
 * buffer of siren_stft_basis_floats() floats (the only host pointer of this ABI; copy it to the device) */
int siren_stft_basis_fill(float* basis_host);
/* floats of siren_spectral.stft_ws / `ws` below for n samples in a batch of `rows` rows (-1: bad shape) */
int64_t siren_stft_workspace_floats(int32_t n, int32_t rows);
/* float offset of a piece of the workspace (-1: unknown): 0 re [T][528], 1 im [T][528], 2 y_mag
 * [T][528], 3 log y_mag [T][528], 4 dF [T][1024], 5 the scalars [32]: {S1, sum|dlog|, Sy, L_stft,
 * 1/(sqrt S1 sqrt Sy), 1/(T 513), mean x, mean y, sum yc^2, sum r^2, L_snr, SNR gradient factor,
 * point loss, mixed loss} */
int64_t siren_stft_ws_offset(int32_t n, int32_t rows, int32_t which);
/* run.py:160 STFT magnitude side: target 0 -- re / im of x and the per-block partials of S1 and
 * sum|dlog| against the stored target; target 1 -- y_mag, log y_mag and Sy of the target (once) */
int siren_stft_forward(const float* x, int32_t n, int32_t rows, const float* basis, float* ws, int32_t target,
                       void* stream);
/* run.py:160 the finished STFT scalars from siren_stft_forward's partials; loss[0] = L_stft (device) */
int siren_stft_loss(int32_t n, int32_t rows, float* ws, float* loss, void* stream);
/* autograd of run.py:160 after siren_stft_forward + siren_stft_loss: g_stft [n] = dL_stft/dx (the
 * transposed GEMM, then a fixed-order gather over frames and reflected images: no atomics) */
int siren_stft_loss_bwd(int32_t n, int32_t rows, const float* basis, float* ws, float* g_stft, void* stream);
/* run.py:126, :165 SNRLoss and its gradient: loss[0] = L_snr, g [n] = dL_snr/dx (both device) */
int siren_snr_loss(const float* x, const float* y, int32_t n, int32_t rows, float* ws, float* loss, float* g,
                   void* stream);

/* run.py:158-185 with the reference's remaining loss options (run.py:126-128, :160-169):
 * loss = (1 - alpha) {MSE | L1 | SNR (batch.loss_mode 0 | 1 | 2)} + alpha L_stft.  The loss is global
 * -- every output sample feeds every gradient -- so the step runs the last layer and the head
 * unfused, the loss kernels above on batch.out, and the backward from the mixed g (left in batch.g,
 * zero on pad rows) exactly as siren_backward runs it; grads.sse[0] receives the FINISHED mixed loss
 * (pass n_total = 1 to siren_apply_update).  The batch must hold the whole signal (n_total ==
 * n_valid, else SIREN_ERR_CONFIG); alpha in [0, 1]; alpha != 0 needs n_valid > 512.  With alpha 0
 * and loss_mode 0 / 1 it is siren_train_step.  (A struct and an entry point of their own: siren_batch
 * and siren_train_step keep their ABI 12 layout and behaviour.) */
typedef struct siren_spectral {
  double alpha;              /* weight of the STFT term */
  const float* stft_basis;   /* siren_stft_basis_floats() floats from siren_stft_basis_fill (alpha != 0) */
  float* stft_ws;            /* siren_stft_workspace_floats(n_valid, rows) floats; with alpha != 0 its target
                                side set once by siren_stft_forward(target, ..., 1) */
} siren_spectral;
int siren_train_step_spectral(const siren_net* net, const siren_grads* grads, siren_batch* batch,
                              const siren_spectral* loss, void* stream);

/* ---- Multi-resolution STFT loss (run.py:127 auraloss.freq.MultiResolutionSTFTLoss(perceptual_weighting=
 * False), the term the reference's 'mrstft' sweeps were fitted with; evaluated at run.py:160) ----------
 * Restated from the published auraloss 0.4.0 defaults: three transforms r = 0, 1, 2 with
 *   n_fft 1024 / 2048 / 512, hop 120 / 240 / 50, win_length 600 / 1200 / 240 (periodic Hann, zero-padded
 *   and centred in the n_fft frame; center, reflect): T_r = 1 + n / hop frames of 513 / 1025 / 257 bins
 *   L_r as L_stft above;  L_mrstft = (L_0 + L_1 + L_2) / 3
 * Only the win_length taps that carry a non-zero window enter the GEMM: per resolution `basis` holds
 * the rows k' = tap - (n_fft - win) / 2 < KWP (win rounded up to 16: 608 / 1200 / 240, zero past win) of
 * v[c][k'][bin] (bin < NBP = 528 / 1040 / 272, zero past the last bin) as [c][k' / 16][bin][k' % 16],
 * then as [c][bin / 16][k'][bin % 16]; resolution 0's 2 * 2 * KWP * NBP floats first, then 1, then 2.
 * n > 1024 (reflect padding of the 2048-point frame is undefined below; else SIREN_ERR_SHAPE), n <= 2^30. */
/* run.py:127, :160 frames of resolution r of an n-sample signal (0: n <= 1024 or r not 0..2) */
int64_t siren_mrstft_frames(int64_t n, int32_t r);
int64_t siren_mrstft_basis_floats(void);
/* run.py:127 the three transforms' tables, fp64 rounded once -- `basis_host` is a HOST buffer of
 * siren_mrstft_basis_floats() floats (copy it to the device) */
int siren_mrstft_basis_fill(float* basis_host);
/* floats of siren_spectral_mr.ws / `ws` below for n samples in a batch of `rows` rows (-1: bad shape) */
int64_t siren_mrstft_workspace_floats(int32_t n, int32_t rows);
/* float offset of a piece of resolution r (-1: unknown): 0 re [T_r][NBP], 1 im, 2 y_mag, 3 log y_mag,
 * 4 dF [T_r][KWP], 5 the scalars [32] (the same for every r): 8 per resolution {S1, sum|dlog|, Sy, L_r,
 * 1/(sqrt S1 sqrt Sy), 1/(T_r bins), -, -}, then {L_mrstft, point loss, mixed loss} */
int64_t siren_mrstft_ws_offset(int32_t n, int32_t rows, int32_t r, int32_t which);
/* run.py:160 magnitude side, one launch per resolution: target 0 -- re / im of x and the per-block
 * partials against the stored target; target 1 -- y_mag, log y_mag and Sy of the target (once) */
int siren_mrstft_forward(const float* x, int32_t n, int32_t rows, const float* basis, float* ws, int32_t target,
                         void* stream);
/* run.py:160 the finished scalars (fp64 on the device) from siren_mrstft_forward's partials:
 * loss[0] = L_mrstft, loss[1..3] = L_0, L_1, L_2 (device) */
int siren_mrstft_loss(int32_t n, int32_t rows, float* ws, float* loss, void* stream);
/* autograd of run.py:160 after siren_mrstft_forward + siren_mrstft_loss: g [n] = dL_mrstft/dx (three
 * transposed GEMMs, then one fixed-order gather: frames ascending, reflected images, resolutions
 * 0, 1, 2 each times 1/3; no atomics) */
int siren_mrstft_loss_bwd(int32_t n, int32_t rows, const float* basis, float* ws, float* g, void* stream);

/* run.py:158-185 with loss = (1 - alpha) {MSE | L1 | SNR} + alpha L_mrstft (run.py:127, :160): composed
 * exactly as siren_train_step_spectral (unfused last layer, the mixed g left in batch.g, zero on pad
 * rows, the finished loss in grads.sse[0]); alpha != 0 needs n_valid > 1024. */
typedef struct siren_spectral_mr {
  double alpha;          /* weight of the multi-resolution STFT term */
  const float* basis;    /* siren_mrstft_basis_floats() floats from siren_mrstft_basis_fill (alpha != 0) */
  float* ws;             /* siren_mrstft_workspace_floats(n_valid, rows) floats; with alpha != 0 its target
                            side set once by siren_mrstft_forward(target, ..., 1) */
} siren_spectral_mr;
int siren_train_step_mrstft(const siren_net* net, const siren_grads* grads, siren_batch* batch,
                            const siren_spectral_mr* loss, void* stream);

/* ---- The spectral losses across micro-batches and ranks (run.py:126-128, :160-169 on a signal that one
 * batch on one GPU does not hold; the sweeps of run.py:439-476 on more than one GPU) ------------------
 * The loss of siren_train_step_spectral / _mrstft in three calls on a signal-length `x` = out [n] that the
 * caller assembled from every micro-batch's (and rank's) siren_forward, target `y` [n], `ws` the
 * whole-signal workspace of siren_{stft,mrstft}_workspace_floats(n, rows) (rows >= n; its target side set
 * once by siren_*_forward(y, ..., 1)).  The caller then runs siren_backward per micro-batch from its slice
 * of g.  loss_mode 0 MSE | 1 L1 | 2 SNR, alpha in [0, 1] (else SIREN_ERR_CONFIG); alpha 0 runs no transform
 * and ignores basis and win.
 *
 * A transform's frames come in blocks of 16; a call runs the frame blocks [win[2 r], win[2 r + 1]) of
 * transform r (win: HOST array of 2 ints for stft, 6 for mrstft), and a block writes its re / im / dF rows
 * and its partial where the whole-signal launch writes them.  siren_*_window gives, for the samples
 * [lo, hi), blocks[0..1] = the blocks to run (every block with a frame over i + n_fft / 2 or one of i's two
 * reflected images, lo <= i < hi) and blocks[2..3] = the blocks owned (first frame t0 with min(t0 hop,
 * n - 1) in [lo, hi)): for any partition of [0, n) the owned ranges partition the blocks, and the run range
 * contains the owned one.  Ranks zero the partials of blocks they do not own and sum the arrays
 * (x + 0 = x: exact); with complete arrays every scalar is the one-batch step's, bit for bit.
 * Status: NULL pointers SIREN_ERR_NULL; n too short, rows < n, a window outside [0, blocks], lo > hi or
 * hi > n SIREN_ERR_SHAPE -- all before any launch. */
/* run.py:128, :160 blocks[4] (HOST) for the samples [lo, hi) of an n-sample signal */
int siren_stft_window(int32_t n, int32_t lo, int32_t hi, int32_t* blocks);
/* run.py:160 where the partials live (-1: bad shape or `which`): 0 float offset in ws of the transform's
 * [2][npart] partials {S1, sum|dlog|}, 1 npart, 2 its frame blocks B, 3 its grid.y (block (b, y) owns the
 * partial y B + b of either row), 4 float offset of the point loss's [8][npart'] partials, 5 npart' */
int64_t siren_stft_signal_parts(int32_t n, int32_t rows, int32_t which);
/* run.py:160-169 partials of the point loss over the whole signal (L1 / MSE per 256 samples, or the SNR
 * sums) and the transform of x on the window */
int siren_stft_signal_forward(const float* x, const float* y, int32_t n, int32_t rows, int32_t loss_mode, double alpha,
                              const float* basis, float* ws, const int32_t* win, void* stream);
/* run.py:160-169 the fp64 finishes over the complete partial arrays; loss[0] = (1 - alpha) point + alpha
 * L_stft (device) */
int siren_stft_signal_finish(int32_t n, int32_t rows, int32_t loss_mode, double alpha, float* ws, float* loss,
                             void* stream);
/* autograd of run.py:160-169 after the finish: the transposed GEMM on the window, then g[lo..hi) =
 * dLoss/dx, indexed by global sample (g [n], device) */
int siren_stft_signal_backward(const float* x, const float* y, int32_t n, int32_t rows, int32_t loss_mode, double alpha,
                               const float* basis, float* ws, const int32_t* win, int32_t lo, int32_t hi, float* g,
                               void* stream);
/* run.py:127, :160 the same for the multi-resolution loss; r = 0, 1, 2 */
int siren_mrstft_window(int32_t n, int32_t r, int32_t lo, int32_t hi, int32_t* blocks);
/* run.py:127, :160 resolution r's partials, `which` as siren_stft_signal_parts */
int64_t siren_mrstft_signal_parts(int32_t n, int32_t rows, int32_t r, int32_t which);
/* run.py:127, :160-169 */
int siren_mrstft_signal_forward(const float* x, const float* y, int32_t n, int32_t rows, int32_t loss_mode,
                                double alpha, const float* basis, float* ws, const int32_t* win, void* stream);
/* run.py:127, :160-169 loss[0] = (1 - alpha) point + alpha L_mrstft */
int siren_mrstft_signal_finish(int32_t n, int32_t rows, int32_t loss_mode, double alpha, float* ws, float* loss,
                               void* stream);
/* autograd of run.py:127, :160-169 */
int siren_mrstft_signal_backward(const float* x, const float* y, int32_t n, int32_t rows, int32_t loss_mode,
                                 double alpha, const float* basis, float* ws, const int32_t* win, int32_t lo,
                                 int32_t hi, float* g, void* stream);

/* autograd addmm dW: slab[s] = partial dZ^T Y over coordinate slice s, tile edge 128/256
 * (0 = siren_dw_tile(rows, hidden)); siren_dw_reduce must get the same tile. */
int siren_inner_bwd_dw(const uint16_t* Y, const uint16_t* dZ, int32_t rows, int32_t hidden,
                       int32_t splits, int32_t tile, float* slab, void* stream);
/* grad (+)= (sum_s slab[s]) * gscale[1]  (gscale NULL = 1) */
int siren_dw_reduce(const float* slab, int32_t splits, int32_t hidden, int32_t tile, float* grad,
                    int32_t accumulate, const float* gscale, void* stream);
int siren_col_reduce(const float* part, int64_t row_stride, int32_t nrows, int32_t ncols, float* out,
                     int32_t out_stride, int32_t accumulate, float* tmp, void* stream);
/* torch.optim.Adam step over a flat fp32 vector (run.py:186) */
int siren_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                    const siren_opt_state* state, void* stream);
/* ReduceLROnPlateau.step(loss) (run.py:187); also increments state->step.  The history slot
 * is state->last_epoch (scheduler steps of this run), not the Adam step: a run resumed from a
 * checkpoint (run.py:84-106) restores the Adam step but builds a fresh scheduler. */
int siren_plateau_step(siren_opt_state* state, const float* sse, double n_total, float* loss_hist,
                       double* lr_hist, int64_t hist_cap, void* stream);
/* fp16 shadows W and W^T of a fp32 [H_out][H_in] weight */
int siren_cast_weight(const float* W, int32_t h_out, int32_t h_in, uint16_t* Wh, uint16_t* WTh,
                      void* stream);

/* ---- unfused fp32 layers: the module API outside the fused step ------------------------
 * A lone SineLayer (models.py:114-120: forward, forward_with_intermediate), nn.Linear, Snake
 * (models.py:235-241) and nn.Tanh -- what SirenWithSnakeTanh.forward_with_activations
 * (models.py:396-423) walks -- in fp32 like the reference (the fused path stores fp16).
 * x [rows][in], W [out][in] (nn.Linear layout), b [out] or NULL; all fp32, row-major. */
enum siren_fp32_act { SIREN_FP32_IDENTITY = 0, SIREN_FP32_SIN = 1, SIREN_FP32_TANH = 2, SIREN_FP32_SNAKE = 3 };
/* pre = omega * (x W^T + b)  (models.py:115 `self.omega_0 * self.linear(input)`; omega 1: nn.Linear) */
int siren_fp32_linear(const float* x, int64_t rows, int32_t in, int32_t out, const float* W, const float* b,
                      float omega, float* pre, void* stream);
/* y = act(x) elementwise over [rows][cols]: sin (models.py:115), tanh, Snake x + sin^2(a x)/a with a [cols] */
int siren_fp32_act(int32_t act, const float* x, int64_t rows, int32_t cols, const float* a, float* y, void* stream);
/* autograd of siren_fp32_act for dL/dy = gy: gx = gy * act'(x); Snake also da [cols] = column sums of
 * gy * dy/da (da_prod: rows*cols floats of scratch, tmp: 64*cols floats; both NULL otherwise) */
int siren_fp32_act_bwd(int32_t act, const float* x, int64_t rows, int32_t cols, const float* a, const float* gy,
                       float* gx, float* da, float* da_prod, float* tmp, void* stream);
/* autograd of siren_fp32_linear for dL/dpre = gpre (overwritten with omega * gpre): gW [out][in] via
 * `splits` split-K slices over the rows into `slab` (splits*out*in floats), gb [out] and gx [rows][in]
 * (either NULL: not computed); tmp: 64*out floats */
int siren_fp32_linear_bwd(const float* x, int64_t rows, int32_t in, int32_t out, const float* W, float omega,
                          float* gpre, float* gx, float* gW, float* gb, float* slab, int32_t splits, float* tmp,
                          void* stream);

/* ---- KAN variant: run.py:92-93 KAN([in, H, H, 1]) of kan.py:169-285 ----------
 * Layer l maps width[l] -> width[l+1] as efficient-KAN's KANLinear (kan.py:6-166) with
 * spline_order 3, SiLU base: out = SiLU(x) base_w^T + B(x) (spline_w*scaler)^T,
 * B = the G + 3 order-3 B-spline bases on the layer's `grid` buffer [in][G + 7], for one grid size
 * G = siren_kan_net.grid_size of 1 .. SIREN_KAN_MAX_GRID in every layer (0 means the default 5, so a
 * zero-initialised struct is a grid-5 net: 8 bases on 12 knots).  A value outside 0 .. 64 is
 * SIREN_ERR_CONFIG before any launch.  Grid 5 runs kernels with its sizes fixed at compile time,
 * every other size the any-grid-size set (kan_general.hip); siren_kan_regrid_* below refits from any
 * of these sizes onto any other (or the same).
 * fp32 throughout.
 * siren_kan_forward / _backward take any last width (out is then [rows][last width]); the fused
 * fit step (siren_kan_train_step) needs last width 1.  Workspace: one caller-owned fp32 buffer of
 * siren_kan_workspace_floats(net, rows, splits) floats (activations, combined weights,
 * gradients of the layer outputs, split-K slabs -- the expansions are never stored). */
#define SIREN_KAN_MAX_LAYERS 8
#define SIREN_KAN_MAX_GRID 64
typedef struct siren_kan_net {
  int32_t n_layers, grid_size;                  /* grid_size: 0 (= 5) or 1 .. SIREN_KAN_MAX_GRID      */
  int32_t width[SIREN_KAN_MAX_LAYERS + 1];
  const float* grid[SIREN_KAN_MAX_LAYERS];      /* [in][G+7]    buffer layers.l.grid        */
  const float* base_w[SIREN_KAN_MAX_LAYERS];    /* [out][in]    layers.l.base_weight        */
  const float* spline_w[SIREN_KAN_MAX_LAYERS];  /* [out][in][G+3] layers.l.spline_weight    */
  const float* scaler[SIREN_KAN_MAX_LAYERS];    /* [out][in]    layers.l.spline_scaler      */
} siren_kan_net;
typedef struct siren_kan_grads {
  float* base_w[SIREN_KAN_MAX_LAYERS];
  float* spline_w[SIREN_KAN_MAX_LAYERS];
  float* scaler[SIREN_KAN_MAX_LAYERS];
  float* sse;                               /* [2] sum of squared errors of valid rows, then (ABI 12)
                                               the fused hand-off's stall flag: both accumulate like the
                                               gradients and ride the same all-reduce */
  float* flat; int64_t flat_len;            /* if flat != NULL and zero_grads: memset   */
} siren_kan_grads;
typedef struct siren_kan_batch {
  int32_t rows, n_valid;    /* rows: any count >= n_valid (no padding needed)      */
  double n_total;           /* global coordinate count (MSE mean denominator)      */
  int32_t splits;           /* split-K slices of the weight-gradient GEMMs (>= 1)  */
  int32_t zero_grads;
  const float* coords;      /* [rows][width[0]]  */
  const float* target;      /* [rows]            */
  float* out;               /* [rows] model output                                */
  float* g;                 /* [rows] dLoss/dout                                  */
  float* ws;                /* workspace, siren_kan_workspace_floats() floats     */
} siren_kan_batch;
int64_t siren_kan_workspace_floats(const siren_kan_net* net, int32_t rows, int32_t splits);
/* run.py:255 model(model_input) for arch='kan' */
int siren_kan_forward(const siren_kan_net* net, siren_kan_batch* batch, void* stream);
/* run.py:158-185 for arch='kan': forward + MSELoss + backward; gradients ACCUMULATE (last width 1) */
int siren_kan_train_step(const siren_kan_net* net, const siren_kan_grads* grads, siren_kan_batch* batch,
                         void* stream);
/* autograd of siren_kan_forward (kan.py:153-166, 268-273) for an arbitrary upstream gradient:
 * batch->g holds dLoss/dout [rows][last width] and batch->ws the workspace of a siren_kan_forward
 * of the same coords, rows and splits; gradients ACCUMULATE (zero_grads + flat: memset first);
 * grad_coords != NULL also receives dLoss/dcoords [rows][width[0]] (grads->sse is not used). */
int siren_kan_backward(const siren_kan_net* net, const siren_kan_grads* grads, siren_kan_batch* batch,
                       float* grad_coords, void* stream);
/* run.py:124-125, :158-185 for arch='kan' under a point loss: loss_mode 0 is nn.MSELoss
 * (siren_kan_train_step, bit for bit), 1 is nn.L1Loss (loss_mode='mae', run.py:161-163): g =
 * sign(out - y) / n_total with torch's sign (0 at out == y) and grads->sse[0] accumulates the sum of
 * |out - y| over the valid rows.  Any other loss_mode: SIREN_ERR_CONFIG, nothing launched. */
int siren_kan_train_step_loss(const siren_kan_net* net, const siren_kan_grads* grads, siren_kan_batch* batch,
                              int32_t loss_mode, void* stream);
/* loss.backward() of run.py:185 for arch='kan' when the loss was computed outside the step (the
 * STFT / SNR losses of run.py:126-128, :160-169 on the whole signal): batch->g holds dLoss/dout
 * [rows] (zero past n_valid) and batch->ws the workspace of a siren_kan_forward of the same coords,
 * rows and splits; last width 1.  A last layer of width <= 64 after a hidden layer runs its rank-1
 * backward in siren_kan_train_step's block partition and summation order (fed that step's g, the
 * gradients are that step's bit for bit); any other shape is siren_kan_backward(grad_coords = NULL).
 * Gradients ACCUMULATE (zero_grads + flat: memset first); grads->sse is not used. */
int siren_kan_step_backward(const siren_kan_net* net, const siren_kan_grads* grads, siren_kan_batch* batch,
                            void* stream);

/* ---- KAN refit: KANLinear.update_grid of kan.py:168-215 and KANLinear.regrid, for one layer ----
 * The reference refits the layer's curves on new knots by a least-squares fit over the batch; regrid
 * (no counterpart in kan.py) does so onto a grid of another size.  A layer fitted on g_old intervals
 * (grid_old [in][g_old + 7], spline_w [out][in][g_old + 3]) is refitted over the rows of x onto g_new
 * intervals: per input i, c_new[i] = G_nn[i]^-1 G_no[i] (spline_w[:, i, :] * scaler[:, i])^T with the
 * Gram matrices G_nn = sum_r b_new(x_ri) b_new(x_ri)^T, (g_new + 3)^2, and G_no = sum_r b_new(x_ri)
 * b_old(x_ri)^T, (g_new + 3) x (g_old + 3), of the fp32 bases on the new and the old knots, summed in
 * fp64 in a fixed order (two calls on the same data agree bit for bit).  update_grid is g_old = g_new
 * with the layer's scaler.  Both sizes are 1 .. SIREN_KAN_MAX_GRID, anything else is SIREN_ERR_CONFIG
 * (-1 from the two size queries) before any launch; 1 <= in, out <= 4096.  The three steps are
 * separate calls; none allocates or synchronises, and none writes a live parameter: the caller copies
 * grid_new and spline_w_new over the layer's buffers once status reads {0, *}.  All pointers are
 * device pointers. */
/* rows that one pass of the Gram kernel's grid covers (more rows loop); -1 on a bad shape */
int64_t siren_kan_regrid_pass_rows(int32_t in, int32_t g_old, int32_t g_new);
/* bytes of the scratch `ws` of siren_kan_regrid_gram over `rows` rows: per row slice and input only
 * the entries that can be non-zero (G_nn's band, G_no's staircase of 4 x 4 blocks), or at 5 -> 5 the
 * dense pair of 8 x 8 matrices, which is smaller; -1 on a bad shape */
int64_t siren_kan_regrid_workspace_bytes(int64_t rows, int32_t in, int32_t g_old, int32_t g_new);
/* kan.py:183-212 op for op in fp32 with g_new for its grid_size: q [g_new + 1][in] holds, per input,
 * x_sorted at torch.linspace(0, rows - 1, g_new + 1, dtype=int64) (any exact selection); grid_new
 * [in][g_new + 7] */
int siren_kan_regrid_knots(const float* q, int32_t in, int32_t g_new, double margin, double grid_eps, float* grid_new,
                           void* stream);
/* gram [in]{G_nn [g_new+3][g_new+3], G_no [g_new+3][g_old+3]} fp64, dense (G_nn symmetric, exact zeros
 * off its band of half-width 3) over x [rows][in]; accumulate != 0 adds to gram's contents
 * (micro-batches of one refit); x is read once */
int siren_kan_regrid_gram(const float* x, int64_t rows, int32_t in, int32_t g_old, int32_t g_new,
                          const float* grid_old, const float* grid_new, int32_t accumulate, double* gram, void* ws,
                          void* stream);
/* kan.py:173-177, :215: spline_w_new [out][in][g_new+3] = fp32(G_nn^-1 G_no (spline_w * scaler)) by a
 * banded fp64 Cholesky factorisation per input; scaler NULL: all ones (the unscaled coefficients).
 * status [2]: the number of rank-deficient inputs (a pivot at or below 2^-40 x the largest diagonal
 * entry of G_nn) and the lowest such index; their rows of spline_w_new are left unwritten.  Needs no
 * scratch */
int siren_kan_regrid_refit(const double* gram, int32_t in, int32_t out, int32_t g_old, int32_t g_new,
                           const float* spline_w, const float* scaler, float* spline_w_new, int32_t* status,
                           void* stream);
/* The (5, 5) case of siren_kan_regrid_* (same kernels, same bits), kept for existing callers: scaler
 * and ws must not be NULL, and siren_kan_grid_refit does not use ws. */
int64_t siren_kan_grid_pass_rows(int32_t in);
int64_t siren_kan_grid_workspace_bytes(int64_t rows, int32_t in);
int siren_kan_grid_knots(const float* q, int32_t in, double margin, double grid_eps, float* grid_new, void* stream);
int siren_kan_grid_gram(const float* x, int64_t rows, int32_t in, const float* grid_old, const float* grid_new,
                        int32_t accumulate, double* gram, void* ws, void* stream);
int siren_kan_grid_refit(const double* gram, int32_t in, int32_t out, const float* spline_w, const float* scaler,
                         float* spline_w_new, int32_t* status, void* ws, void* stream);

/* ---- per-launch HIP-event profiling of the fused path (bench.py) --------------------
 * siren_profile_enable(n) creates 2n hipEvents; while enabled every launch made by
 * siren_train_step / siren_backward / siren_forward / siren_apply_update (and the KAN
 * entry points, kinds 8..11) is bracketed
 * by events on its stream (eager launches only; not meant for graph capture).
 * siren_profile_read sums the elapsed time of all records of one kind (synchronises). */
enum siren_prof_kind {
  SIREN_PROF_FIRST_FWD = 0, SIREN_PROF_INNER_FWD = 1, SIREN_PROF_HEAD = 2, SIREN_PROF_BWD_DW = 3,
  SIREN_PROF_BWD_DX = 4, SIREN_PROF_BWD_DX0 = 5, SIREN_PROF_REDUCE = 6, SIREN_PROF_UPDATE = 7,
  /* KAN variant (siren_kan_train_step / siren_kan_forward): KAN_FWD the fused forward layers
   * (and the inference head); KAN_DW the last layer's training pass (forward, MSE gradient,
   * backward) and the first layer's weight gradient (+ slab reduces); KAN_DX the hidden layers'
   * one-pass backward (dW and dX); KAN_MISC the small rest */
  SIREN_PROF_KAN_FWD = 8, SIREN_PROF_KAN_DW = 9, SIREN_PROF_KAN_DX = 10, SIREN_PROF_KAN_MISC = 11,
  /* the last hidden layer fused with the head, the loss gradient and the head backward
   * (siren_train_step with SIREN_OPT_HEAD_FUSE; counted apart from INNER_FWD) */
  SIREN_PROF_HEAD_FWD = 12,
  /* the STFT / SNR loss kernels and the loss mix (siren_train_step_spectral) */
  SIREN_PROF_LOSS = 13,
  SIREN_PROF_NKINDS = 14
};
/* tuning knobs for in-process A/B measurement (process-global; 0 = automatic):
 * SIREN_OPT_NT_TILE / SIREN_OPT_TN_TILE = 128 or 256 forces the GEMM tile edge;
 * SIREN_OPT_NT_PIPE = 256x256 NT GEMM K-loop: -1 automatic (4), 0 BK 64 one tile per block,
 * 1 BK 64 persistent double buffer, 4 BK 64 persistent with two wave groups in ping-pong; the
 * plain forward (no head) also takes the one-wave-per-SIMD measurement kernels 5 (128x256 tiles,
 * the epilogue under the next tile's MFMAs), 6 (256x256, BK 32, 4-stage ring) and 7 (pipe 5's K loop
 * with the epilogue at the tile's end), bit-identical to 4; other modes take 4;
 * SIREN_OPT_TN_PIPE = -1..4 selects the 256x256 dW K-loop (-1 automatic = 4; 0: BK 64 double
 * buffer, 1: BK 32 4-slot ring, 2: BK 32 5-slot ring, 3: BK 64 ping-pong in 16-MFMA phases,
 * 4: BK 64 ping-pong in 32-MFMA segments);
 * SIREN_OPT_NT_GRID = persistent NT grid size (0 = one block per CU; tests use small
 * values so every block walks several tiles);
 * SIREN_OPT_NT_DIAG = measurement-only NT ablations, accepted only by libraries built with
 *   -DSIREN_DIAG (__graft_entry__.build_diagnostic; the product library returns
 *   SIREN_ERR_CONFIG for any non-zero value); results are WRONG while set: bit 0 reads the X
 *   operand from the first 4 row bands only (L2-resident operand), bit 3 from the first 256 row bands
 *   (an X of 128 MB: Infinity-Cache-resident, not L2); ping-pong K-loop only: bit 2
 *   reads W from column tile 0 only (L2-resident W), bit 9 runs no tiles, bit 10 skips the
 *   epilogue (its compute and stores);
 * SIREN_OPT_NT_QUEUE = 1 (default): the ping-pong NT GEMM's persistent blocks take their tiles
 * from the caller's tile-queue set (siren_batch.tileq; 8 shard heads, agent-scope atomics) in the
 * forward modes, 2: in every mode, 0: never (the static walk b, b + G, ...).  Results are
 * identical.  (Options 5 and 7, the round-2 start stagger and X L2-prefetch distance, were
 * measured neutral or slower and retired with their kernels: they return SIREN_ERR_CONFIG.)
 * SIREN_OPT_HB_FAULT = measurement / test hook of the fused last layer's hand-off, accepted only by
 *   -DSIREN_DIAG libraries (product: SIREN_ERR_CONFIG for non-zero): bit 0 -- the blocks of column
 *   tile 1 never publish their head partials; value >> 8 (when non-zero) -- the wait's poll limit
 *   (default 2^23 polls of s_sleep 1, ~1.3 s).  Used to drive the timeout branch in tests.
 * SIREN_OPT_HEAD_FUSE = 1 (default): siren_train_step runs a sine last layer on 256x256
 * ping-pong tiles as one launch with the head, the loss gradient and the head backward
 * (dZ_L is written instead of Y_L / C_L; the backward scale S then comes from a bound of
 * max|g| known before the forward); 0: separate forward, head_loss and head_bwd launches.
 * SIREN_OPT_KAN_GENERAL = 0 (default): a KAN of grid_size 5 runs its own kernels; 1: it runs the
 * any-grid-size kernels that every other grid size runs (tests and measurement: the two sets
 * side by side on one net). */
enum siren_option {
  SIREN_OPT_NT_TILE = 0, SIREN_OPT_TN_TILE = 1, SIREN_OPT_NT_PIPE = 2, SIREN_OPT_TN_PIPE = 3,
  SIREN_OPT_NT_GRID = 4, SIREN_OPT_NT_DIAG = 6, SIREN_OPT_NT_QUEUE = 8, SIREN_OPT_HEAD_FUSE = 9,
  SIREN_OPT_HB_FAULT = 10, SIREN_OPT_KAN_GENERAL = 11
};
int siren_set_option(int32_t option, int32_t value);
int siren_profile_enable(int32_t max_records);
int siren_profile_reset(void);
/* bit k set: launches of kind k are bracketed (default all).  bench.py times its steps with only
 * the dominant kind bracketed, so the events cost the timed region ~2 records per launch of that
 * kind instead of ~2 per launch of the step (measured: all kinds add 2-13% to a step). */
int siren_profile_mask(uint32_t kinds);
int siren_profile_read(int32_t kind, double* total_ms, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* SIREN_HIP_H */
