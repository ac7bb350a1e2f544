/*
 * rcv.h -- C ABI of librcv.so, the MI355X (gfx950) implementation of the RoboCupVision
 * ROBO-UNet / U-Net training hot path.
 *
 * The reference (szemenyeim/RoboCupVision) has no FFI of its own: its hot path bottoms out in
 * PyTorch ATen operators called from model.py / train.py.  This header is therefore the boundary
 * a maintainer would bind *instead of* those operator calls; every entry point names the
 * reference call site it replaces (file:line into the reference repository).
 *
 * Conventions
 *   - extern "C", plain pointers and integers only.  No torch / C++ types cross the boundary.
 *   - Every function returns 0 on success, a negative RCV_E_* code on failure; the text of the
 *     last failure on the calling thread is returned by rcv_last_error().  Nothing throws.
 *   - All pointers are device pointers BORROWED for the duration of the call (they must stay valid
 *     until the work enqueued on `stream` has completed).  The library never allocates device
 *     memory: outputs and workspaces are passed in; sizes come from rcv_op_workspace().
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).  All work is
 *     enqueued asynchronously on it; nothing here synchronises the device (graph-capture safe).
 *   - Activations are fp32 NHWC ([N][H][W][C], C contiguous).  The network input (images) and the
 *     network output (logits) are fp32 NCHW, as the reference's callers hand over / expect.
 *   - All reductions are fixed-order (no float atomics): results are bitwise reproducible.
 *
 * Execution model: the host describes each kernel invocation as one `rcv_op` record; a whole
 * forward or backward pass is an array of records executed by ONE call to rcv_run() (one host
 * call per pass instead of one per layer; the records are plain data and may be cached).
 * The named entry points further down are conveniences that fill a record and run it.
 */
#ifndef RCV_H
#define RCV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCV_VERSION 100

/* error codes */
#define RCV_OK            0
#define RCV_E_ARG        -1   /* bad argument / unsupported shape */
#define RCV_E_HIP        -2   /* a HIP runtime call failed        */
#define RCV_E_UNSUPPORTED -3

typedef struct rcv_handle rcv_handle;

int  rcv_create(int device, rcv_handle** out);
/* A handle without a device, for hosts that only lay out buffers: rcv_op_workspace / rcv_op_kernel_label answer for a chip with
 * `num_cus` compute units (256 on MI355X); every call that would enqueue work fails with RCV_E_ARG. */
int  rcv_create_planner(int num_cus, rcv_handle** out);
int  rcv_destroy(rcv_handle* h);
const char* rcv_last_error(void);
int  rcv_version(void);
/* Multiprocessor (CU) count of the handle's device; used by callers to size split-K. */
int  rcv_num_cus(const rcv_handle* h);

/* ------------------------------------------------------------------------------------------ */
/* Operation records                                                                           */
/* ------------------------------------------------------------------------------------------ */

/* kinds */
enum {
  RCV_OP_CONV        = 1,  /* 3x3 gather convolution (implicit GEMM on MFMA)                     */
  RCV_OP_TCONV       = 2,  /* 3x3 stride-2 transposed convolution, pad 1, output_padding 1       */
  RCV_OP_WGRAD       = 3,  /* 3x3 filter gradient, split over pixels, partials to workspace      */
  RCV_OP_WGRAD_REDUCE= 4,  /* fixed-order sum of WGRAD partials -> parameter-layout gradient     */
  RCV_OP_PACK        = 5,  /* parameter tensors -> kernel filter layout, table driven            */
  RCV_OP_BN_FINALIZE = 6,  /* batch statistics -> scale/shift (+ running stats)                  */
  RCV_OP_BN_EVAL     = 7,  /* running statistics -> scale/shift; row 3 = bias folded through the BatchNorm: (p[X4] ? bias : 0)*scale + shift */
  RCV_OP_BN_BWD      = 8,  /* backward reductions -> (A,B,C) constants, dgamma, dbeta            */
  RCV_OP_COMBINE     = 9,  /* up = relu(t*s+h) + (r*s2+h2)          (decoder skip add)           */
  RCV_OP_CLS_FWD     = 10, /* 1x1 classifier, NHWC in (8 or 16 channels) -> NCHW logits, 1..8 classes (model.py:411; numClass = 5 - nb - ng - nr - nl, train.py:301) */
  RCV_OP_CLS_BWD     = 11, /* classifier backward (dgrad + wgrad + dbias) from NCHW dlogits, same shapes */
  RCV_OP_CE_FWD      = 12, /* weighted softmax cross-entropy forward (+argmax, +#correct)        */
  RCV_OP_CE_BWD      = 13, /* d loss / d logits                                                  */
  RCV_OP_POOL_FWD    = 14, /* 2x2/2 max-pool of (r*s+h)                                          */
  RCV_OP_POOL_BWD    = 15, /* max-pool backward (+skip gradient, + BN backward reductions)       */
  RCV_OP_ADAM_L1     = 16, /* fused Adam step with decay*sign(p) L1 gradient over a flat buffer  */
  RCV_OP_MEMSET      = 17, /* zero a float buffer                                                */
  RCV_OP_CONV1X1     = 18, /* generic 1x1 convolution NHWC -> NHWC/NCHW (LabelProp classifier)   */
  RCV_OP_ADD_SLICE   = 19, /* x[..., 0:Ca] += affine(a)   (LabelProp top skip, model.py:565)     */
  RCV_OP_MATERIALIZE = 20, /* out = load(in)  (a block's normalised output as a plain tensor)    */
  RCV_OP_BWD_STATS   = 21, /* out = g[.., aux0:aux0+cout] (g has cin channels per pixel, 0 = cout); partial rows of the BN-backward sums */
  RCV_OP_CONFUSION   = 22, /* counts[n][pred][label] += 1 per pixel (int32, accumulating)            */
  RCV_OP_DICE_FWD    = 23, /* weighted soft-Dice loss forward (+argmax, +#correct)   model.py:5-43 */
  RCV_OP_DICE_BWD    = 24, /* d loss / d logits of the Dice loss                                  */
  RCV_OP_NHWC_TO_NCHW= 25, /* out[n][c][p] = in[n][p][c] + bias[c], c < cout <= cin (3x3 classifier tail) */
  RCV_OP_NCHW_TO_NHWC= 26, /* out[n][p][c] = c < cin ? in[n][c][p] : 0, cout channels per pixel     */
  RCV_OP_SGD         = 27, /* torch.optim.SGD(momentum, weight_decay) over a flat buffer (trainer.py:176-178) */
  RCV_OP_NOP         = 28, /* nothing is launched (a slot of an op list whose work was folded into a later record)       */
  RCV_OP_WGRAD_REDUCE_BATCH = 29, /* RCV_OP_WGRAD_REDUCE of several layers in ONE launch: p[RCV_P_IN] -> rcv_reduce_job[i[RCV_I_COUNT]]
                                   * (device memory); same fixed summation order per layer as the single form                  */
  RCV_OP_POOL_CLS_FWD = 30, /* pooled patch-classification head (model.py:255-266,403-414): k x k max (i[AUX0] = 2 / 4, floor) or plane
                             * mean (i[AUX0] = 0) of load(r), optional Dropout2d keep-scale p[X0] = float[N][C], 1x1 classifier
                             * (1..8 classes) -> NCHW logits; the pooled features [N][HO][WO][C] go to p[X1] (csrc/pool_cls.hip) */
  RCV_OP_POOL_CLS_BWD = 31, /* its backward: dW (p[X2]), db (p[X3]) and d loss / d load(r) NHWC (first arg-max of a max window; the
                             * mean's share of every pixel), RCV_F_RESID, RCV_STATS_BWD_ENC / _DEC partial rows of the producer  */
  RCV_OP_OBJECT_MATCH = 32, /* object-detection counts of test.py:28-89 (rcv_object_match; csrc/objdet.hip): i[N], i[H], i[W], i[COUT] = C,
                             * i[COUNT] = K, i[INMODE] / i[INMODE2] = element bytes of p[IN] pred / p[IN2] target (1 = uint8, 8 = int64);
                             * p[X0] / p[X1] = HOST double[K] IoU / distance thresholds (read when enqueued), p[OUT] = counts, p[PART] =
                             * workspace, i[NPART] = its size in 256-byte units (filled by rcv_op_workspace)                          */
  RCV_OP_LP_TAIL_FWD = 33,  /* LabelProp's tail in training mode (model.py:563-567: x = upConv3(x); x[:,0:8] += top; classifier(x)), one launch
                             * (csrc/lp_tail.hip): logits = W v + b, v[c] = relu(t[c]*c0[c] + c1[c]) + (c < i[AUX1] ? f(r[c]) : 0) -- the ReLU is
                             * taken BEFORE the skip is added (the out-of-place form of that line).  Slots as RCV_OP_CLS_FWD with RCV_F_FUSED_UP
                             * (required): i[CIN] = 16, i[COUT] = 1..8 classes, p[IN] = t (NHWC, 16 channels), p[IN_C] = its constants, p[X3] = skip
                             * tensor r (NHWC, i[AUX1] channels: a multiple of 4, 4..16), p[X4] = its constants, i[AUX0] = its load mode (PLAIN /
                             * AFFINE / AFFINE_RELU), p[W], p[BIAS], p[OUT] = NCHW logits.  RCV_F_FUSED_CE: also the weighted cross entropy, as
                             * documented at that flag (same partial rows and finalisation as RCV_OP_CE_FWD)                               */
  RCV_OP_LP_TAIL_BWD = 34,  /* its backward, one launch + the fixed-order row reduction.  Slots as RCV_OP_CLS_BWD with RCV_F_FUSED_UP (required),
                             * i[STATS] = RCV_STATS_BWD_DEC (required), i[AUX0] / i[AUX1] / p[X3] / p[X4] as the forward, p[EPI_AUX] = t, p[EPI_C] =
                             * its constants (row 2 = batch mean), p[IN2] = NCHW logits gradient -- or, with RCV_F_FUSED_CE, the int64 target and
                             * the other operands of that flag; outputs: p[OUT] = g = W^T dlogits (NHWC, 16 channels: the gradient of the decoder
                             * block's output, its statistics rows in p[PART]), p[IN_AUX] = g[..., 0:i[AUX1]] as a dense NHWC tensor (the skip
                             * tensor's gradient: handed to the data-gradient launch of its other consumer as RCV_F_RESID), p[X1] = dW
                             * [COUT][16], p[X2] = db                                                                                         */
  RCV_OP_LP_BATCH = 35,     /* batch assembly of labelPropTrain.py:162-193 (rcv_labelprop_batch; csrc/lp_tail.hip): i[N] = B frame pairs, i[CIN] =
                             * channels per frame, i[H], i[W], i[COUT] = classes (5); p[IN] = images float[B][2][C][H][W], p[IN2] = labels
                             * int64[B][2][H][W], p[OUT] = inputs float[2B][H][W][8] (NHWC), p[X0] = targets int64[2B][H][W]              */
  RCV_OP_BATCH_PREP = 36,   /* the loader's per-image work of dataset.py:107-133 for a whole batch (rcv_batch_prep; csrc/batch_prep.hip): i[N] = B,
                             * i[H] / i[W] = source Hs / Ws, i[HO] / i[WO] = output H / W, i[CIN] / i[COUT] = taps per output column / row of the
                             * frame tables, i[INMODE2] = label element bytes (1 = uint8, 4 = int32), i[AUX0] = train (0 / 1), i[AUX1] = maskLabel
                             * flags (1 = nb, 2 = nr, 4 = ng, 8 = nl); p[IN] = frames uint8[B][Hs][Ws][3], p[IN2] = labels [B][Hs][Ws], p[X1] / p[X2] =
                             * frame tables of x / y, p[X3] / p[X4] = label index tables of x / y, p[X5] = normalisation table float[3][256],
                             * p[IN_C] = parameter rows float[B][8] (train only), p[OUT] = imgs float[B][3][H][W], p[X0] = targets int64[B][H][W] */
  RCV_OP_CLS_LABEL = 37,    /* the inference form of the classifier tails (detect.py:131-133: `_, predClass = torch.max(pred, 1)`, then Colorize):
                             * no logits are stored and no target is read; p[OUT] = class map uint8[N][H][W] (the FIRST maximum of the logits in
                             * class order, the rule of RCV_F_FUSED_CE's arg-max: a NaN never wins, an all-NaN pixel is class 0), p[X0] = colour
                             * image uint8[N][H][W][3] = palette[class] or NULL, p[X1] = palette uint8[8][3] in device memory (required iff
                             * p[X0]).  i[N], i[H], i[W], i[CIN], i[COUT] = 1..8 classes; i[INMODE] = the source form:
                             *   0 features: the 1x1 classifier is applied, slots exactly as RCV_OP_CLS_FWD (p[IN], p[W] = [COUT][CIN], p[BIAS] or
                             *     NULL, CIN 8 / 16; with RCV_F_FUSED_UP p[IN_C], p[X3], p[X4], i[AUX0] = the skip's load mode, i[AUX1] = its channel
                             *     count, 0 = CIN); the logits are formed in the order of RCV_OP_CLS_FWD, so the map is bit for bit the arg-max of
                             *     the logits that record writes;
                             *   1 logits: p[IN] is NHWC with i[CIN] floats per pixel (a multiple of 4, >= COUT), the first COUT of them logits;
                             *     p[BIAS] (or NULL) is added, p[W] is not read (the tail of the 3x3 classifier, in place of RCV_OP_NHWC_TO_NCHW);
                             *   2 class map: p[IN] is a class map of i[INMODE2] bytes per element (1 = uint8, 8 = int64); only the colour image is
                             *     produced (a class outside [0, 8) is black, as Colorize leaves unmatched pixels 0); p[OUT] is not written.
                             * i[COUNT] = store shape: 0 = the library's choice, 1 = one byte / three bytes per pixel and lane, 4 = the labels
                             * and colours of four neighbouring pixels gathered into one / three dword stores (csrc/cls_label.hip)            */
  RCV_OP_FRAME_PREP = 38,   /* RCV_OP_BATCH_PREP with train = 0 for frames that have no labels (detect.py:125-130; rcv_frame_prep): the same slots
                             * and the same resize / normalise code; no label is read, no label table and no target: p[IN2], p[X0], p[X3], p[X4]
                             * and i[INMODE2], i[AUX0], i[AUX1] are not looked at.  p[OUT] is bit for bit what the other record writes             */
  RCV_OP_BNN_STAGE_FWD = 39, /* one stage of the BNN-L / BNN-M-C patch classifiers (model.py:590-592, 615-618; csrc/bnn.hip), one launch:
                             * out = relu(maxpool_{k,2}(dropout2d(conv_{KxK, pad P, stride 1}(x) + bias))).  i[N], i[H], i[W] = input plane, i[CIN]
                             * (3 / 8 / 16), i[COUT] (4 / 8 / 16), i[AUX0] = K (3 / 5 / 8), i[COUNT] = P (0 / 1 / 3 / 4), i[AUX1] = pool k (0 = no
                             * pool, 2, 4: k x k windows at stride 2, floor), i[HO], i[WO] = output plane, i[INMODE] = RCV_LOAD_NCHW (the network
                             * input, 3 channels) or RCV_LOAD_PLAIN (NHWC); flags RCV_F_RELU, RCV_F_OUT_NCHW (BNN-M-C's classifier writes the
                             * logits).  p[IN] = x, p[W] = filter [COUT][CIN][K][K] (the parameter itself), p[BIAS], p[X0] = Dropout2d keep-scale
                             * float[N][COUT] (0 or 1/(1-p)) or NULL, p[OUT], p[X1] = uint8[N][HO][WO][COUT]: the window offset of the FIRST
                             * maximum in row-major window order (aten's rule), or NULL where no backward follows; p[X2] = uint8[N][HO][WO]: the
                             * FIRST maximum over the output channels of the values p[OUT] gets (the class map of `torch.max(pred, 1)`), or
                             * NULL; with it p[OUT] may be NULL                                                                      */
  RCV_OP_BNN_STAGE_BWD = 40, /* its backward, one launch + the fixed-order row reduction: d loss / d conv is GATHERED over the <= 4 windows
                             * that contain a pixel (no atomics).  Slots as the forward, and p[IN] = d loss / d out, p[IN_AUX] = out (with
                             * RCV_F_RELU), p[EPI_AUX] = x, p[OUT] = dx NHWC (RCV_LOAD_PLAIN only; NULL for the network input), p[X2] = dW
                             * [COUT][CIN][K][K], p[X3] = db, p[PART] = i[NPART] partial rows of COUT*CIN*K*K + COUT floats                    */
  RCV_OP_BNN_HEAD_FWD = 41,  /* BNN-L's head (model.py:593), one launch: logits = Wc relu((Wfc x + bfc) * keep) + bc per pixel.  i[N], i[H], i[W] =
                             * head plane, i[CIN] = 16, i[COUNT] = 512 hidden units, i[COUT] = 1..8 classes; p[IN] = x NHWC, p[W] = Wfc [512][16],
                             * p[BIAS] = bfc, p[X0] = Dropout keep-scale float[N][H][W][512] (0 or 2) or NULL, p[X1] = Wc [COUT][512], p[X2] = bc,
                             * p[OUT] = NCHW logits or NULL, p[X3] = uint8[N][H][W] FIRST maximum of those logits or NULL (at least one of the two) */
  RCV_OP_BNN_HEAD_BWD = 42,  /* its backward, one launch + the row reduction: p[IN] = NCHW logits gradient, p[EPI_AUX] = x, p[W], p[BIAS], p[X0],
                             * p[X1] as the forward; p[OUT] = dx NHWC [N][H][W][16], p[X2] = dWfc, p[X3] = dbfc, p[X4] = dWc, p[X5] = dbc,
                             * p[PART] = i[NPART] partial rows (rcv_op_workspace)                                                        */
  RCV_OP_CE_NORM = 43,       /* the normaliser of the weighted cross entropy, sum_p w[target_p], from the targets alone, left as partial rows:
                             * i[N], i[H], i[W], i[COUT] = classes (1..8), p[IN2] = int64 target, p[X0] = class weights or NULL, p[PART] =
                             * float[i[NPART]] (rcv_op_workspace), one value per workgroup.  Grid, pixel -> thread mapping and summation order
                             * are those of RCV_OP_CLS_FWD with RCV_F_FUSED_CE: row b is bit for bit column 1 of that op's partial row b, and
                             * the rows summed in RCV_OP_CE_FWD's finalisation order give its loss_out[1].  Runs ahead of RCV_OP_CLS_STEP   */
  RCV_OP_CLS_STEP = 44,      /* the training step's turn from forward to backward at the fused 1x1 classifier: RCV_OP_CLS_FWD and RCV_OP_CLS_BWD,
                             * both with RCV_F_FUSED_UP | RCV_F_FUSED_CE, in ONE pass over t, the skip tensor and the targets, then one launch
                             * for the fixed-order reductions (dW, db and the loss).  8 input channels, 1..8 classes.  Slots exactly as
                             * RCV_OP_CLS_BWD with both flags (required; i[STATS] = RCV_STATS_BWD_DEC required): p[EPI_AUX] = t, p[EPI_C] = its
                             * constants, p[X3] / p[X4] / i[AUX0] = the skip tensor, its constants, its load mode, p[W], p[BIAS], p[IN2] = int64
                             * target, p[X0] = class weights or NULL, p[IN2_AUX] = d loss scalar, p[OUT] = d_up, p[X1] = dW, p[X2] = db, p[PART] =
                             * i[NPART] partial rows (rcv_op_workspace: the backward op's layout) -- and the forward's outputs: p[RESID] = NCHW
                             * logits, p[IN_AUX] = uint8 arg-max or NULL, p[IN2_C] = float[i[NPART]][3] loss partial rows, p[X5] = float[4]
                             * loss_out (WRITTEN here, as RCV_OP_CE_FWD writes it), p[IN_C] = the float[i[NPART]] rows of an RCV_OP_CE_NORM
                             * record over the same targets and weights, run before this one.  Every output and every partial row is bit
                             * for bit what the two records write                                                                      */
  RCV_OP_PRUNE = 45,         /* the magnitude-pruning mask builders (model.py:45-57 pruneModelNew, :621-642 pruneModel, :644-672 pruneModel2) for
                             * every weight tensor of a model in ONE launch (rcv_prune; csrc/prune.hip): p[IN] = rcv_prune_job[i[COUNT]] in
                             * device memory, i[AUX0] = the rule (RCV_PRUNE_*).  One workgroup per job, integer counts only: nothing is reduced
                             * across workgroups and no result depends on scheduling.  The weights are zeroed in place, the masks and the
                             * result rows of the jobs are written                                                                     */
  RCV_OP_OBJECTS = 46,       /* the objects of a class map (rcv_find_objects; csrc/objects.hip): per image and class 1..C-1 the 8-connected
                             * components that pass the class's area rules, largest first.  i[N], i[H], i[W], i[COUT] = C (2..8), i[COUNT] = M
                             * = max_objects (1..16), i[INMODE] = element bytes of p[IN] (1 = uint8, 8 = int64), i[AUX0] = kernel form (0 = the
                             * library's choice by shape, 1 = the general multi-launch form, 2 = the single-launch form with the union-find in
                             * LDS, refused where the plane does not fit; both forms write identical bytes); p[IN] = class map [N][H][W],
                             * p[OUT] = rows int32 [N][C-1][M][8], p[X0] = counts int32 [N][C-1][4], p[X1] = HOST double[C-1] min_ratio, p[X2] =
                             * HOST int32[C-1] min_area, p[X3] = HOST int32[C-1] cap (the three read when enqueued), p[PART] = workspace,
                             * i[NPART] = its size in 256-byte units (filled by rcv_op_workspace)                                       */
  RCV_OP_RGB_PREP = 47,      /* the loader of trainer.py:75-123 (and pruner.py, labelPropTrain.py, tester.py, makeLPImages.py, classTrainer.py,
                             * objDetEval.py) for a whole batch (rcv_rgb_prep; csrc/rgb_prep.hip): Scale, the two flips, torchvision's PIL
                             * ColorJitter, rgb2yuv, ToTensor, Normalize([.5,0,0],[.5,.5,.5]), and the label's Scale, flips and maskLabel.
                             * i[N] = B, i[H] / i[W] = source Hs / Ws, i[HO] / i[WO] = output H / W, i[CIN] / i[COUT] = taps per output column /
                             * row of the frame tables, i[INMODE2] = label element bytes (1 = uint8, 4 = int32; 0 = no labels: the patch chain),
                             * i[AUX0] = train (0 / 1), i[AUX1] = maskLabel flags, i[COUNT] = 1 when a parameter row may hold a contrast
                             * operation (the statistics launch runs), 0 promises that none does (a row that does anyway blends towards 0);
                             * p[IN] = frames uint8[B][Hs][Ws][3], p[IN2] = labels [B][Hs][Ws], p[X1] / p[X2] = frame tables of x / y, p[X3] / p[X4] =
                             * label index tables of x / y (the four as RCV_OP_BATCH_PREP), p[IN_C] = parameter rows float[B][12] (train only),
                             * p[OUT] = imgs float[B][3][H][W], p[X0] = targets int64[B][H][W], p[PART] = uint32[i[NPART]]: one partial sum of L
                             * per workgroup of the statistics launch (i[NPART] filled by rcv_op_workspace; 0 unless train and i[COUNT])     */
  RCV_OP_FARNEBACK = 48,     /* dense optical flow of B frame pairs by Farnebaeck's polynomial expansion (rcv_farneback_flow; csrc/flow.hip;
                             * transform.py:185-187 optFlow).  i[N] = B, i[H], i[W], i[CIN] = bytes per pixel of the frames (1 = gray, 3 = RGB:
                             * gray = (4899 R + 9617 G + 1868 B + 8192) >> 14 is formed on load), i[COUNT] = levels (0..4), i[AUX0] = winsize
                             * (odd, 1..15), i[AUX1] = iterations (1..64), i[STRIDE] = poly_n (5 or 7), i[DIL] = cv2's flags word (0 only),
                             * f[0] = pyr_scale (0.5 only), f[1] = poly_sigma; p[IN] = prev uint8[B][H][W](x3), p[IN2] = next, p[OUT] = flow
                             * float[B][2][H][W] (channel 0 = dx along columns, 1 = dy along rows), p[PART] = workspace, i[NPART] = its size in
                             * 256-byte units (filled by rcv_op_workspace)                                                              */
  RCV_OP_REMAP_LABELS = 49,  /* a class map moved through a flow (rcv_update_labels; csrc/flow.hip; transform.py:189-198 updateLabels): out[y][x]
                             * = in[rint(y + flow[1])][rint(x + flow[0])] inside the plane, 0 outside; fp32 sums, rint = half to even.  i[N],
                             * i[H], i[W], i[INMODE] = element bytes (1 = uint8, 8 = int64); p[IN] = class map [N][H][W], p[IN2] = flow
                             * float[N][2][H][W], p[OUT] = class map [N][H][W] (not p[IN])                                              */
  RCV_OP_OBJECT_PATCHES = 50,/* the boxes of an RCV_OP_OBJECTS result cut out of the full-resolution frames and brought to the patch
                             * classifiers' input (rcv_object_patches; csrc/patches.hip): Pillow's 8-bit BILINEAR resize of every box, then
                             * rgb2yuv + Normalize([.5,0,0],[.5,.5,.5]), one launch, one workgroup per slot.  i[N], i[H] / i[W] = Hs / Ws of the
                             * frames, i[HO] / i[WO] = H / W of the class map the boxes live in (1..Hs / 1..Ws), i[COUT] = C - 1 (classes with
                             * boxes), i[COUNT] = M (rows per class), i[AUX0] / i[AUX1] = patch Sh / Sw (1..64 each), i[CIN] = margin >= 0 in
                             * class-map pixels; p[IN] = frames uint8[N][Hs][Ws][3], p[IN2] = rows int32[N][C-1][M][8] (columns 0..3 = x, y,
                             * w, h are read), p[X0] = counts int32[N][C-1][4] (column 3 = emitted is read), p[OUT] = images float
                             * [N (C-1) M][3][Sh][Sw], p[X1] = bytes uint8[N (C-1) M][Sh][Sw][3] or NULL; both outputs are written for every
                             * slot (zeros past the emitted count: nothing needs pre-zeroing).  No workspace.  Refused when planned: a count
                             * < 1, a patch side outside 1..64, margin < 0, a map larger than the frames, W Ws or H Hs past 32 bits,
                             * coefficient tables (2 + ceil(in / out) 2 + 1 int32 per output index and axis) beyond the LDS of a workgroup */
  RCV_OP_RESIZE_U8 = 51,     /* the resize stage of RCV_OP_BATCH_PREP alone (rcv_resize_u8; csrc/batch_prep.hip): the bytes that record feeds its
                             * normalisation lookup, and the labels gathered and NOT masked -- what a device-resident dataset keeps, since
                             * everything random comes after them.  i[N] = B, i[H] / i[W] = source Hs / Ws, i[HO] / i[WO] = output H / W, i[CIN] /
                             * i[COUT] = taps per output column / row of the frame tables, i[INMODE2] = label element bytes in (1 = uint8, 4 =
                             * int32; 0 = no labels: p[IN2], p[X0], p[X3], p[X4] are not looked at), i[INMODE] = label element bytes out (1 =
                             * uint8: the low byte of an int32 label, the 4 -> 1 narrowing for planes whose values are <= 255; 4 = int32);
                             * p[IN] = frames uint8[B][Hs][Ws][3], p[IN2] = labels [B][Hs][Ws], p[X1] / p[X2] = frame tables of x / y, p[X3] /
                             * p[X4] = label index tables of x / y (the four as RCV_OP_BATCH_PREP), p[OUT] = bytes uint8[B][H][W][3] (NHWC),
                             * p[X0] = labels [B][H][W].  H == Hs and W == Ws: a plain copy (or narrowing / widening) of both.  Same tiles and
                             * the same staged / through-the-cache choice as RCV_OP_BATCH_PREP.  No workspace.  Refused when planned: what
                             * RCV_OP_BATCH_PREP refuses, and a label width out other than 1 or 4                                       */
  RCV_OP_BATCH_PREP_IDX = 52,/* RCV_OP_BATCH_PREP whose image b is store[index[b]] (rcv_batch_prep_indexed): the slots of that record, and
                             * i[COUNT] = N images in the store p[IN] = frames uint8[N][Hs][Ws][3] / p[IN2] = labels [N][Hs][Ws], p[IN_AUX] =
                             * index [B] in DEVICE memory, i[INMODE] = its element bytes (4 = int32, 8 = int64), p[EPI_AUX] = int32 counter in
                             * device memory.  i[N] = B = rows of the index, of p[IN_C], of p[OUT] and of p[X0].  Bit for bit the outputs of
                             * RCV_OP_BATCH_PREP on the gathered images (the same arithmetic in the same order), in both kernel forms.  An
                             * index outside [0, N) is tested before it forms an address: that image is written as zeros with targets 0 and
                             * the counter is incremented once (an atomic add; the caller zeroes it and reads it when it likes) -- nothing
                             * is read out of bounds, nothing synchronises.  Refused when planned: what RCV_OP_BATCH_PREP refuses (the pixel
                             * limit counts the store), N < 1, an index element size other than 4 or 8, a null index or counter          */
  RCV_OP_RGB_PREP_IDX = 53,  /* RCV_OP_RGB_PREP whose image b is store[index[b]] (rcv_rgb_prep_indexed; csrc/rgb_prep.hip; the loader of
                             * trainer.py:75-123 fed from a resident store): the slots of that record, and i[STRIDE] = N images in the store
                             * (i[COUNT] stays that record's statistics switch) p[IN] = frames uint8[N][Hs][Ws][3] / p[IN2] = labels
                             * [N][Hs][Ws], p[IN_AUX] = index [B] in DEVICE memory, i[INMODE] = its element bytes (4 = int32, 8 = int64),
                             * p[EPI_AUX] = int32 counter in device memory.  i[N] = B = rows of the index, of p[IN_C], of p[OUT], of p[X0] and
                             * of the partial sums (i[NPART] = B x workgroups per image, as RCV_OP_RGB_PREP).  Bit for bit the outputs of
                             * RCV_OP_RGB_PREP on the gathered images, in both kernel forms and both launches.  An index outside [0, N) is
                             * tested before it forms an address, in both launches: the statistics launch writes a 0 partial, the main
                             * launch writes that image as zeros with targets 0 and increments the counter once (an atomic add) -- nothing
                             * is read out of bounds, nothing synchronises.  Refused when planned: what RCV_OP_RGB_PREP refuses (the pixel
                             * limit counts the store), N < 1, an index element size other than 4 or 8, a null index or counter          */
  RCV_OP_LP_PAIR_PREP = 54,  /* LabelProp's input straight from a resident store (rcv_lp_pair_prep; csrc/rgb_prep.hip): per pair the loader of
                             * labelPropTrain.py:36-66 on both frames and the assembly of labelPropTrain.py:162-193, i.e. RCV_OP_LP_BATCH of
                             * RCV_OP_RGB_PREP_IDX with ONE parameter row per pair, Y only.  i[N] = B pairs, i[H] / i[W] = size of the store's
                             * images, i[HO] / i[WO] = the network's size (must equal i[H] / i[W]: only the no-resize form is built),
                             * i[COUT] = classes (5), i[STRIDE] = N images in the store, i[INMODE2] = label element bytes (1 / 4), i[INMODE] =
                             * element bytes of the pairs (4 / 8), i[AUX0] = train, i[COUNT] = statistics switch as RCV_OP_RGB_PREP; p[IN] =
                             * frames uint8[N][H][W][3], p[IN2] = labels [N][H][W], p[IN_AUX] = pairs [B][2] in DEVICE memory (store indices
                             * of frame a, frame b), p[EPI_AUX] = int32 counter, p[IN_C] = parameter rows float[B][12] (train only), p[OUT] =
                             * inputs float[2B][H][W][8] (NHWC, 16-byte aligned), p[X0] = targets int64[2B][H][W], p[PART] =
                             * uint32[i[NPART]], i[NPART] = 2B x workgroups per frame (0 unless train and i[COUNT]).  A pair with either
                             * index outside [0, N): both samples zeros, targets 0, counted once                                       */
  RCV_OP_CONV5 = 55,         /* 5x5 gather convolution, stride 1, pad 2 (rcv_conv5x5; csrc/conv5.hip): the classifier convolution of
                             * Classifier(kernelSize=5) / UltClassifier(size=5) (model.py:256-267, model.py:403-414) and, with the filter packed
                             * flipped and transposed, its data gradient.  Slots, load transform, flags (RCV_F_BIAS / _RELU / _RESID) and
                             * statistics rows exactly as RCV_OP_CONV; i[STRIDE] = i[DIL] = 1, i[HO] = i[H], i[WO] = i[W]; p[W] = the
                             * [25][CIN][16] filter an RCV_OP_PACK5 record writes.  Channel pairs: CIN 8 / 16 -> COUT 8 (the class channels
                             * padded to 8: at most 8 classes), CIN 8 -> COUT 8 / 16 (data gradient); i[INMODE] PLAIN / AFFINE / AFFINE_RELU.
                             * Everything else is refused when planned.  One partial row per 256-pixel tile                            */
  RCV_OP_WGRAD5 = 56,        /* its filter and bias gradient (rcv_wgrad5x5), split over pixels: slots as RCV_OP_WGRAD; p[IN] = the conv's input
                             * (i[CIN] = 8 / 16 channels, i[INMODE] as above), p[IN2] = the output gradient NHWC with i[COUT] = 8 padded class
                             * channels (i[INMODE2] = PLAIN), RCV_F_BIAS = also the bias gradient; p[PART] = float[i[NSPLIT]][25 * 8 * 16 + 8]
                             * (i[NSPLIT] filled by rcv_op_workspace): per split the partial filter [25 taps][8][16] and the partial bias [8] */
  RCV_OP_WGRAD5_REDUCE = 57, /* fixed-order sum (split 0, 1, ...) of RCV_OP_WGRAD5's partial rows -> p[OUT] = dW [COUT][CIN][5][5], p[BIAS] = db
                             * [COUT] or NULL; i[CIN] = 8 / 16, i[COUT] = 1..8 classes, i[NSPLIT], p[PART]                              */
  RCV_OP_PACK5 = 58,         /* p[IN] = parameter [COUT][CIN][5][5] (i[CIN] = 8 / 16, i[COUT] = 1..8) -> p[OUT] = float[25][rows][16], zero
                             * padded: forward rows = CIN, out[t][ci][co] = w[co][ci][t]; with RCV_F_FLIP the data gradient's filter, rows =
                             * 8, out[t][co][ci] = w[co][ci][24 - t]                                                                    */
  RCV_OP_LP_INPUT = 59,      /* LabelProp's input from a PREDICTION of the previous frame (rcv_lp_input; csrc/lp_input.hip; makeLPImages.py:94-102,
                             * validLabelProp.py:116-135, the commented prior of labelPropTrain.py:179): per pixel of sample s,
                             * [Ycur, Yprev, Ycur - Yprev, prior_0 .. prior_4].  i[N] = B samples, i[H], i[W], i[CIN] = channels per frame (only
                             * channel 0 is read), i[COUT] = classes (5), i[INMODE] = the prior's form: 1 = class map uint8[B][H][W], 8 = class
                             * map int64[B][H][W] (labelToPred; a value outside [0, 5), decided on all 64 bits, gives -1 in all five channels
                             * and is never used as an index), 4 = logits float[B][5][H][W] (2 * softmax - 1: m = max z, e_c = expf(z_c - m),
                             * S = (((e_0 + e_1) + e_2) + e_3) + e_4, 2 * (e_c / S) - 1, IEEE division).  i[AUX0] = pairing: 0 = stream form,
                             * p[IN] = current frames float[B][C][H][W], p[IN2] = previous frames float[B][i[AUX1]][H][W] (i[AUX1] = 0: C
                             * channels), sample s reads frame s of both and prior[s]; 1 = pair form, p[IN] = float[B/2][2][C][H][W] seen as
                             * B frames (B even, p[IN2] not read, i[AUX1] = 0 or C), sample s reads frames s, s ^ 1 and prior[s ^ 1]
                             * (labelPropTrain.py:181-182; the targets of that script are the label tensor itself: none are written).
                             * p[X0] = the prior, p[OUT] = inputs float[B][H][W][8] (NHWC, 16-byte aligned), p[X1] = Ycur as a dense plane
                             * float[B][H][W] or NULL.  Refused when planned: classes != 5, another prior form or pairing, odd B in the
                             * pair form, B / C / H / W < 1, an operand of 2^31 elements or more                                        */
  RCV_OP_CLS_VALID = 60,     /* the validation form of the classifier tails (rcv_cls_valid; csrc/cls_valid.hip; valid() of train.py:97-178:
                             * `criterion(model(imgs), targets)`, `torch.max(pred, 1)` and the mask loops of train.py:136-153): the class, the
                             * loss terms and the confusion bin of every pixel from its logits in registers; no logits are stored.  Slots and
                             * source forms as RCV_OP_CLS_LABEL: i[N], i[H], i[W], i[CIN], i[COUT] = 1..8 classes, i[INMODE] 0 = features
                             * (p[IN], p[W], p[BIAS] or NULL, CIN 8 / 16; with RCV_F_FUSED_UP p[IN_C], p[X3], p[X4], i[AUX0], i[AUX1]),
                             * 1 = NHWC logits of i[CIN] floats per pixel plus p[BIAS], 2 = p[IN] is a uint8 class map: only the counts are
                             * produced, no loss (p[PART] NULL and i[NPART] 0, refused otherwise).  p[IN2] = targets int64[N][H][W]; p[X0] =
                             * class weights float[COUT] or NULL (no colour image is produced here); p[PART] = float[i[NPART]][3] partial rows
                             * (rcv_op_workspace) of sum w*nll, sum w, #correct, the columns of RCV_OP_CE_FWD; p[X2] = int32[N][COUT][COUT]
                             * counts[image][pred][label], ACCUMULATED as RCV_OP_CONFUSION accumulates; p[OUT] = class map uint8[N][H][W] or
                             * NULL (forms 0 and 1).  The class is the first maximum (a NaN never wins), bit for bit RCV_OP_CLS_LABEL's.  A
                             * target outside [0, COUT), decided on the int64 value, has weight 0 and counts in no bin.  For 8-channel
                             * features and for logits the rows are bit for bit those RCV_OP_CE_FWD forms from the logits RCV_OP_CLS_FWD /
                             * RCV_OP_NHWC_TO_NCHW write (same grid, pixel -> thread mapping and summation order); with 16 channels four
                             * lanes share a pixel and the rows are sums over other pixel sets (the loss agrees to rounding)          */
  RCV_OP_VALID_FOLD = 61,    /* folds one batch into the running validation state and clears the counts it read (rcv_valid_fold; one
                             * workgroup).  p[IN] = counts int32[N][C][C] of RCV_OP_CLS_VALID (zero afterwards); the batch loss: p[IN2] =
                             * partial rows with i[NPART] > 0, summed in RCV_OP_CE_FWD's finalising order to the fp32 loss, OR p[X0] = a
                             * device float with i[NPART] = 0 (exactly one of the two, checked when planned); i[N], i[H], i[W], i[COUT] = C;
                             * p[OUT] = state double[76]: [0] += (double)loss (train.py:131 `losstotal += loss.item()`), [1] += 1 (batches),
                             * [2] += N (images), [3] += N*H*W (pixels), [4 + c] = iou_sum[c]: one thread per class adds, image by image in
                             * index order, inter / union with inter = n[c][c], union = sum_l n[c][l] + sum_p n[p][c] - inter, 1.0 where
                             * union is 0 (train.py:148-153); [12 + 8 * pred + label] += sum over the images of n[pred][label]        */
  RCV_OP_PW = 62,            /* pointwise (1x1) convolution between feature maps (rcv_conv_pw; csrc/conv_pw.hip; model.py:345 ConvSep.conv_1x1,
                             * model.py:366 trConvSep.conv): out[n][p][co] = sum_ci load(in)[n][p][ci] * W[co][ci], NHWC, over the N*H*W pixels
                             * (any count: the tail is guarded).  i[CIN] / i[COUT] = channels of p[IN] / p[OUT], multiples of 8 in 8..128;
                             * p[W] = the PARAMETER itself, [COUT][CIN] -- or, with RCV_F_TRANSPOSED_SRC, [CIN][COUT]: the data gradient of the
                             * layer whose parameter it is (the same product with the filter transposed); nothing is packed.  p[X0] = a
                             * per-output-channel factor of the filter or NULL (the inference BatchNorm fold).  i[INMODE] PLAIN / AFFINE /
                             * AFFINE_RELU / GRAD_ENC / GRAD_DEC with p[IN_C], p[IN_AUX]; RCV_F_BIAS / _RELU / _RESID and the statistics rows
                             * (i[STATS], p[EPI_AUX], p[EPI_C], p[PART]) exactly as RCV_OP_CONV; one partial row per pixel tile, every row
                             * written.  i[STRIDE], i[DIL], i[HO], i[WO] are not looked at                                                */
  RCV_OP_PW_WGRAD = 63,      /* its filter gradient (rcv_wgrad_pw), split over pixels: dW[co][ci] = sum_p load(dy)[p][co] * load(x)[p][ci].
                             * p[IN] = x (i[CIN] channels, i[INMODE] PLAIN / AFFINE / AFFINE_RELU, p[IN_C]), p[IN2] = dy (i[COUT] channels,
                             * i[INMODE2] PLAIN / GRAD_ENC / GRAD_DEC, p[IN2_AUX], p[IN2_C]); p[PART] = float[i[NSPLIT]][COUT][CIN]
                             * (i[NSPLIT] filled by rcv_op_workspace): every row is written whole, each element once; no atomics.  i[AUX0] =
                             * 16x16 filter blocks per wave at most (4 or 8; 0 = the library's default, 4): speed only                    */
  RCV_OP_PW_WGRAD_REDUCE = 64, /* fixed-order sum (row 0, 1, ...; float64, rounded once) of those rows -> p[OUT] = dW [COUT][CIN]; i[CIN],
                             * i[COUT], i[NSPLIT], p[PART]                                                                              */
  RCV_OP_CROSS_PACK = 65,    /* two 1-D filters -> one dense 3x3 filter in parameter layout with a cross of non-zero taps, which the 3x3
                             * records then read like any parameter (csrc/conv_pw.hip).  p[OUT] = dense float[D0][D1][3][3], D0 = i[COUT],
                             * D1 = i[CIN]; i[AUX0] = 0: cat(conv_nx1(x), conv_1xn(x)) (model.py:342-349), p[IN] = [D0/2][D1][3][1] in the
                             * centre column of rows < D0/2, p[IN2] = [D0/2][D1][1][3] in the centre row of the others; i[AUX0] = 1:
                             * trconv1x3(x) + trconv3x1(x) (model.py:367-376), p[IN] = [D0][D1][1][3] in the centre row, p[IN2] =
                             * [D0][D1][3][1] in the centre column, the centre tap their sum.  Every element of the dense filter is written */
  RCV_OP_CROSS_GRAD = 66,    /* the gather that undoes it on a gradient: p[IN] = dense gradient float[D0][D1][3][3], p[OUT] / p[X0] = the
                             * gradients of the first / second 1-D filter; with i[AUX0] = 1 the centre tap's gradient goes to both        */
  RCV_OP_CLS_PROBA = 67,     /* the softmax form of the classifier tails (rcv_cls_proba; csrc/cls_proba.hip): the [softmax] section that
                             * closes every exported net.cfg, and the confidence gate of a pseudo-label.  Source forms 0 and 1 of
                             * RCV_OP_CLS_LABEL, slot for slot: i[N], i[H], i[W], i[CIN], i[COUT] = 1..8 classes, i[INMODE] 0 = features
                             * (p[IN], p[W], p[BIAS] or NULL, CIN 8 / 16; with RCV_F_FUSED_UP p[IN_C], p[X3], p[X4], i[AUX0], i[AUX1]),
                             * 1 = NHWC logits of i[CIN] floats per pixel plus p[BIAS]; form 2 is refused.  No logits are stored.  Per
                             * pixel: m = the first maximum of the logits z in class order (a NaN never wins), cls = its index, e_c =
                             * expf(z_c - m), S = ((e_0 + e_1) + e_2) + ... in class order, p_c = e_c / S (IEEE division, no fast
                             * intrinsics; RCV_OP_LP_INPUT's softmax).  Outputs, each optional, at least one (checked at launch), a NULL
                             * slot is not written: p[X0] = probabilities float[N][COUT][H][W]; p[OUT] = class map uint8[N][H][W], bit
                             * for bit RCV_OP_CLS_LABEL's; p[X1] = confidence float[N][H][W] = p[cls], the float stored in p[X0]; p[X2]
                             * = pseudo-label int64[N][H][W] = cls where that stored confidence >= f[0], else -100 (the ignore value
                             * of the losses: any target outside [0, COUT)).  A NaN logit gives whatever the expressions give (NaN
                             * probabilities for the pixel, the class from the other logits, pseudo-label -100); a NaN f[0] gives
                             * -100 everywhere.  No atomics; every element is written once by a fixed lane                            */
  RCV_OP_CLS_CALIB = 68,     /* the calibration form of the classifier tails (rcv_cls_calib; csrc/cls_calib.hip): counts per predicted
                             * class, label and confidence bin, from which the host reads what every threshold of a sweep keeps; nothing
                             * per pixel is stored.  Source forms 0 and 1 slot for slot as RCV_OP_CLS_PROBA (i[N], i[H], i[W], i[CIN],
                             * i[COUT] = C = 1..8, i[INMODE], p[IN], p[W], p[BIAS]; with RCV_F_FUSED_UP p[IN_C], p[X3], p[X4], i[AUX0],
                             * i[AUX1]): class cls and confidence cf are formed by RCV_OP_CLS_PROBA's expressions, so cf is bit for bit
                             * the float that record stores in p[X1].  Form 2: p[IN] = a stored class map uint8[N][H][W] and p[X1] = a
                             * stored confidence map float[N][H][W] (i[CIN] is not looked at).  RCV_F_FUSED_UP belongs to form 0.
                             * p[IN2] = targets int64[N][H][W] or NULL; p[X0] = edges float[K] in device memory, K = i[COUNT] in 1..32,
                             * ascending (not checked: see the bin rule); p[X2] = state int64[K + 1][C][C + 3], ACCUMULATED into.
                             * Per pixel: bin = #{ j : cf >= edges[j] } -- a count of K comparisons on the fp32 confidence, the very
                             * comparison of RCV_OP_CLS_PROBA's pseudo-label gate, in [0, K] whatever the edges hold; the labelled pixels
                             * with bin > j are those f[0] = edges[j] keeps there.  q = (uint32)(cf * 2^26): the product is exact in
                             * fp32, the conversion truncates (cf <= 0 gives 0, cf >= 64 gives 2^32 - 1; a softmax confidence lies in
                             * (0, 1]).  With target t, 0 <= t < C decided on the int64 value: state[bin][cls][t] += 1 and
                             * state[bin][cls][C + 1] += q; otherwise, and with p[IN2] NULL: state[bin][cls][C] += 1 and
                             * state[bin][cls][C + 2] += q.  A pixel whose confidence is NaN counts nowhere; in form 2 neither does a
                             * pixel whose class byte is >= C.  Each workgroup counts in LDS and adds its non-zero entries with 64-bit
                             * integer atomics: every sum is an integer sum, so the state is bitwise reproducible in any order      */
  RCV_OP_MAP_FILTER = 69     /* a class map cleaned by a windowed class count and one decision rule (rcv_map_filter; csrc/map_filter.hip):
                             * the majority vote of labelExtraction.py:70-89 __filterMask (switched off there at :46) and the morphology
                             * test.py:41 leaves commented in front of connectedComponents (cv2.MORPH_CLOSE, 3x3).  i[N], i[H], i[W],
                             * i[COUT] = C = 1..8, i[COUNT] = window k = 1..15, i[INMODE] = element bytes of the map (1 = uint8, 8 =
                             * int64), i[AUX0] = rule (RCV_MF_*), i[AUX1] / i[STRIDE] / i[DIL] = the rule's parameters (at the rules),
                             * i[INMODE2] = 1 when p[IN] is a bit map (the *_FINISH rules), else 0; p[IN] = the windowed input [N][H][W],
                             * p[IN2] = the original map of the *_FINISH rules, p[OUT] = the result [N][H][W], never p[IN] (halo pixels
                             * are read after their neighbours are written), p[X0] = int32[N] or NULL: the number of pixels of each
                             * image whose value changed is ADDED to it (not by the *_BITS rules).  A pixel value v is a class when
                             * 0 <= v < C (decided on the int64 value), else void: 255, -100, anything else.  Per pixel: h[c] = the
                             * number of in-image pixels of class c in the window, whose offsets on each axis are -(k / 2) ... k - 1 -
                             * (k / 2) (k = 4: -2 ... +1, the reference's range(-2, 2, 1)); n = the number of in-image pixels of the
                             * window; a void pixel counts in no h[c] but in n.  A pixel the rule leaves alone keeps every bit of its
                             * value.  Integer arithmetic only, no workspace; the morphological rules (RCV_MF_ERODE_BITS and above) take
                             * odd k only: with a symmetric window opening is anti-extensive and closing extensive                    */
};

/* i[RCV_I_AUX0] of RCV_OP_MAP_FILTER: the decision rule.  S = i[AUX1], a bit set of classes < C; v = the pixel's own value */
enum {
  RCV_MF_MAJORITY = 0,       /* i[STRIDE] = min_major >= 1, i[DIL] = min_own >= 0, i[AUX1] = fill_void (0 / 1).  m = max h, a = the lowest
                              * class attaining it, own = h[v] for a class, 0 for void.  A void pixel keeps its value unless fill_void;
                              * otherwise out = a if m >= min_major or (v is a class and own < min_own), else v.  The reference's
                              * filter is k = 4, min_major = 15, min_own = 7                                                        */
  RCV_MF_ERODE = 1,          /* i[STRIDE] = fill (0..255 for uint8 maps, any int32 for int64 maps): a class pixel with v in S and h[v] < n
                              * becomes fill; everything else is unchanged                                                          */
  RCV_MF_ERODE_BITS = 2,     /* map -> bit map uint8[N][H][W]: bit c set iff c in S, v == c and h[c] == n                               */
  RCV_MF_DILATE_BITS = 3,    /* map -> bit map uint8[N][H][W]: bit c set iff c in S and h[c] > 0                                        */
  RCV_MF_OPEN_FINISH = 4,    /* p[IN] = bit map (RCV_MF_ERODE_BITS'), p[IN2] = original map -> map; the counts are taken per bit of the bit
                              * map (bits outside S are not counted).  i[STRIDE] = fill: a class pixel with v in S whose count for v is 0
                              * becomes fill; everything else is unchanged                                                          */
  RCV_MF_CLOSE_FINISH = 5    /* p[IN] = bit map (RCV_MF_DILATE_BITS'), p[IN2] = original map -> map.  i[DIL] = O, a bit set of classes < C
                              * plus bit 8 for void: the lowest c in S whose count equals n and for which v == c or v in O gives out =
                              * c; without one out = v                                                                              */
};
/* the tile of one workgroup of RCV_OP_MAP_FILTER (tests build planes past it) */
#define RCV_MAP_FILTER_TILE_H 32
#define RCV_MAP_FILTER_TILE_W 64

/* i[RCV_I_AUX0] of RCV_OP_PRUNE: how the threshold of a tensor is chosen */
enum {
  RCV_PRUNE_MAX_RATIO = 0,   /* pruneModelNew: thresh = fp32(max|w| * fp32(ratio)); zero |w| < thresh; mask = |w| < thresh                   */
  RCV_PRUNE_STD_SEARCH = 1,  /* pruneModel: thresh starts at the sample standard deviation (float64 accumulation, two passes, rounded to fp32)
                              * and is stepped by fp32(1.025) / fp32(0.975) until lower <= 100 * #(|w| < thresh) / #(w != 0) <= upper; at most
                              * RCV_PRUNE_MAX_ITER steps (the reference's loop need not terminate)                                      */
  RCV_PRUNE_SMALLEST_K = 2   /* pruneModel2: zero the `amount` smallest |w| (exact radix select on the bit pattern; among equal magnitudes at
                              * the boundary the LOWEST flat indices go: torch.topk leaves that choice open); mask = (w == 0) afterwards  */
};
#define RCV_PRUNE_MAX_ITER 4096
/* rcv_prune_job.result[3] */
#define RCV_PRUNE_ST_OK       0
#define RCV_PRUNE_ST_NO_END   1   /* rule 1: the search did not settle within RCV_PRUNE_MAX_ITER steps; the tensor is left untouched  */
#define RCV_PRUNE_ST_ALL_ZERO 2   /* rule 1: no non-zero weight (the reference's ZeroDivisionError); untouched                          */
#define RCV_PRUNE_ST_BAD_JOB  3   /* a job rcv_prune_check refuses reached the device; untouched                                       */

/* how an operand is produced from memory while it is staged (rcv_op.i[RCV_I_INMODE] etc.) */
enum {
  RCV_LOAD_PLAIN    = 0,   /* v = x                                                              */
  RCV_LOAD_AFFINE   = 1,   /* v = x*c0[ch] + c1[ch]                (BatchNorm apply of producer) */
  RCV_LOAD_GRAD_ENC = 2,   /* v = aux>0 ? c0*x + c1 + c2*aux : 0   (BN-bwd then ReLU-bwd)        */
  RCV_LOAD_GRAD_DEC = 3,   /* v = c0*(aux*c3+c4>0 ? x : 0) + c1 + c2*aux   (ReLU-bwd then BN-bwd)*/
  RCV_LOAD_NCHW     = 4,   /* v = x, tensor is NCHW (network input image, <= 4 channels)           */
  RCV_LOAD_AFFINE_RELU = 5 /* v = max(x*c0+c1, 0)               (conv->BN->ReLU producer)        */
};

/* epilogue statistics written as per-workgroup partial rows [n_part][2][C] */
enum {
  RCV_STATS_NONE   = 0,
  RCV_STATS_FWD    = 1,    /* sum v, sum v*v                     (BatchNorm batch statistics)    */
  RCV_STATS_BWD_ENC= 2,    /* sum g, sum g*(e-mean)     e = epi_aux, mean = epi_c row 2 (BN backward, conv->ReLU->BN)   */
  RCV_STATS_BWD_DEC= 3     /* sum g*m, sum g*m*(e-mean) m = (e*c0+c1>0)                 (BN backward, convT->BN->ReLU) */
};

/* flag bits (rcv_op.flags) */
#define RCV_F_BIAS      1u    /* add bias[co]                                                     */
#define RCV_F_RELU      2u    /* clamp at zero after bias                                         */
#define RCV_F_RESID     4u    /* add resid[...] (same shape as the output) before stats/store     */
#define RCV_F_OUT_NCHW  8u    /* CONV1X1 / CLS: store NCHW                                        */
#define RCV_F_FLIP      16u   /* PACK: reverse the 3x3 taps                                       */
#define RCV_F_TRANSPOSED_SRC 32u /* PACK / WGRAD_REDUCE: parameter is [Cin][Cout][3][3] (convT)  */
#define RCV_F_ARGMAX    64u   /* CE_FWD: also write argmax mask and count correct pixels          */
#define RCV_F_TRAINING  128u  /* BN_FINALIZE: update running stats                                */
#define RCV_F_FUSED_UP   512u  /* CLS_FWD / CLS_BWD: the input is the decoder output relu(t*c0+c1) + f(r), formed on the fly from t (p[IN] resp.
                               * p[EPI_AUX]), its constants (p[IN_C] resp. p[EPI_C]), the skip tensor p[X3], its constants p[X4], i[AUX0] = its
                               * load mode -- RCV_OP_COMBINE is then not needed for this value                                             */
#define RCV_F_FUSED_CE   1024u /* with RCV_F_FUSED_UP: CLS_FWD also produces the weighted cross entropy (p[IN2] = int64 target, p[X0] = class weights or
                               * NULL, p[PART], p[X1] = float[4] loss_out as RCV_OP_CE_FWD, p[X2] = uint8 arg-max or NULL); CLS_BWD forms d loss / d logits
                               * itself (p[IN2] = target, p[X0] = class weights, p[BIAS], p[X5] = loss_out, p[IN2_AUX] = d loss scalar): the
                               * logits gradient tensor and RCV_OP_CE_BWD are not needed                                              */
#define RCV_F_SIDE_STREAM (1u << 16) /* rcv_run: enqueue this op on the handle's side stream (forked from / joined to the caller's
                                      * stream inside the call): ops off the critical path, e.g. the filter gradients of backward */
#define RCV_F_MFMA_FP32 (1u << 17) /* CONV / TCONV / WGRAD: contract on the fp32 matrix instructions (v_mfma_f32_16x16x4_f32) only.  Without it the
                                      wide layers form their fp32 products on the bf16 matrix pipe from operands split EXACTLY into three
                                      bf16 values (six partial products per multiply-add, fp32 accumulate; error <= the fp32 chain's against
                                      fp64, csrc/wgrad_bf3.hip): same results to fp32 rounding, 2-2.5 x the matrix rate.  Part of the plan key. */
#define RCV_F_STREAM_OUT (1u << 18) /* CONV / TCONV / COMBINE: store the output tensor with streaming (nontemporal) stores whatever its size.  Without
                                      the flag the library decides from the tensor's size (rcv_set_stream_min_mb, default 128 MiB; 0 = never):
                                      a tensor that large is gone from the caches before its consumer asks for it.  Honoured by the narrow
                                      families (convs_mfma, convn_bf3), the first layer and combine / concat; the others ignore it.  Results
                                      are bit for bit the same either way.  Not part of the plan key. */
#define RCV_F_STREAM_PW  (1u << 19) /* COMBINE (WGRAD, CONV: accepted, not honoured by a kernel yet): read the pointwise operands -- read once per
                                      element, no halo -- with streaming loads whatever their size; without the flag by size, as above */
#define RCV_F_CONCAT    256u  /* COMBINE: out[..,0:C] = relu(t*s+h), out[..,C:2C] = f(r)  (v2 skip concat, model.py:507) */
/* bits 20..22: profiling ablations of diagnostic builds (skip staging / skip the contraction); the shipped kernels of the wide
 * layers ignore them */
#define RCV_F_DBG_NOSTAGE (1u << 20)
#define RCV_F_DBG_NOSKIP  (1u << 22)
#define RCV_F_DBG_NOMFMA  (1u << 21)
#define RCV_F_DBG_NOEPI   (1u << 23)   /* filter gradient: skip the partial-filter stores (ablation timing only) */

/* integer slots */
enum {
  RCV_I_N = 0, RCV_I_H, RCV_I_W,          /* spatial dims of the gathered (input) tensor          */
  RCV_I_CIN, RCV_I_COUT,
  RCV_I_HO, RCV_I_WO,                     /* spatial dims of the output tensor                    */
  RCV_I_STRIDE, RCV_I_DIL,
  RCV_I_INMODE,                           /* RCV_LOAD_* of operand `in`                           */
  RCV_I_INMODE2,                          /* WGRAD: RCV_LOAD_* of the pointwise operand           */
  RCV_I_STATS,                            /* RCV_STATS_*                                          */
  RCV_I_NPART,                            /* rows of `part` (filled by rcv_op_workspace)          */
  RCV_I_NSPLIT,                           /* WGRAD: pixel splits (filled by rcv_op_workspace)     */
  RCV_I_COUNT,                            /* element / job count for table driven ops             */
  RCV_I_AUX0, RCV_I_AUX1,                 /* TCONV: AUX0 = 1 when the filter is packed in the merged-parity layout */
  RCV_I__N = 20
};

/* pointer slots */
enum {
  RCV_P_IN = 0,      /* gathered operand                                                          */
  RCV_P_IN_AUX,      /* second tensor of a GRAD_* load                                            */
  RCV_P_IN_C,        /* per-channel constants of the load: float[5][C] planar (c0..c4)            */
  RCV_P_W,           /* packed filter / parameter                                                 */
  RCV_P_BIAS,
  RCV_P_OUT,
  RCV_P_RESID,
  RCV_P_EPI_AUX,     /* tensor e of the BWD statistics                                            */
  RCV_P_EPI_C,       /* float[3][C]: (c0, c1) = the mask of RCV_STATS_BWD_DEC, row 2 = the batch mean both backward kinds centre e about */
  RCV_P_PART,        /* partial rows                                                              */
  RCV_P_IN2,         /* WGRAD: pointwise operand                                                  */
  RCV_P_IN2_AUX,
  RCV_P_IN2_C,
  RCV_P_X0, RCV_P_X1, RCV_P_X2, RCV_P_X3, RCV_P_X4, RCV_P_X5,   /* kind specific            */
  RCV_P__N = 20
};

typedef struct rcv_op {
  int32_t  kind;
  uint32_t flags;
  int32_t  i[RCV_I__N];
  float    f[8];
  void*    p[RCV_P__N];
} rcv_op;

/* Fills op->i[RCV_I_NPART] / [RCV_I_NSPLIT] for the tiling the library will use and returns
 * the bytes of the `part` workspace the op needs (0 if none).  This query (and rcv_op_kernel_label) REFUSES exactly the records a
 * launch would refuse for their shape -- channel counts, load modes, flag combinations; operand pointers and workspace row counts are
 * the only things checked at launch alone -- so a caller can validate a whole op list when it builds it (RCV_E_ARG + rcv_last_error). */
int rcv_op_workspace(const rcv_handle* h, rcv_op* op, size_t* part_bytes);

/* Enqueue ops[0..n) in order on `stream`.  The handle's device is made current for the duration of the call (and the caller's
 * current device restored): `stream` must belong to the handle's device. */
int rcv_run(rcv_handle* h, const rcv_op* ops, int n, void* stream);

/* rcv_run with options.  RCV_RUN_NO_JOIN: leave the side stream (RCV_F_SIDE_STREAM ops) un-joined when the call returns; the caller
 * joins it later with rcv_join_side (data-parallel training runs the backward list in slices and lets the communication stream,
 * not the compute stream, wait for the filter gradients of a slice). */
#define RCV_RUN_NO_JOIN 1u
int rcv_run_ex(rcv_handle* h, const rcv_op* ops, int n, void* stream, uint32_t run_flags);
/* Make `stream` wait for everything enqueued on the handle's side stream so far (no-op if none exists). */
int rcv_join_side(rcv_handle* h, void* stream);

/* Profiling aid (not for the training path: it creates HIP events and synchronises the stream):
 * runs ops[0..n) like rcv_run with a hipEvent pair around every op and writes the elapsed
 * milliseconds of op k to ms[k] (host memory). */
int rcv_run_timed(rcv_handle* h, const rcv_op* ops, int n, void* stream, float* ms);

/* Filter layout the library wants for an RCV_OP_CONV record before its filter is packed: 0 = [9 taps][Cin][Cout] (rcv_pack_job.merged
 * 0), 2 = Winograd F(2x2,3x3) transformed [16][Cin][Cout] (rcv_pack_job.merged 2), 3 / 4 / 5 = the split-bf16 layouts of
 * rcv_pack_job.merged (1.5 x the bytes of the plain layout); the record then carries the answer in i[RCV_I_AUX0].  RCV_OP_CONV: the wide
 * (Cin % 32 == 0, >= 64 channels) stride-1 layers whose grid covers the chip answer 3 (2 when the record carries RCV_F_MFMA_FP32), the
 * wide stride-2 layers (Cin % 16 == 0, >= 32; Cout >= 64) answer 5, the 16 / 32-channel layers whose fp32 form is matrix-pipe bound 3;
 * RCV_OP_TCONV records in the merged form (i[RCV_I_AUX0] = 1) answer 4 where the split-bf16 narrow kernel is the faster one;
 * `force` != 0 answers 2 for every shape the Winograd kernel can run. */
int rcv_op_filter_layout(const rcv_handle* h, const rcv_op* op, int force);

/* The streaming hints the library applies to `op`: RCV_F_STREAM_OUT | RCV_F_STREAM_PW bits (>= 0), decided from the record's own
 * N*H*W*C against the handle's threshold, or forced by the record's flags; negative RCV_E_* for a record the planner refuses. */
int rcv_op_stream_hints(const rcv_handle* h, const rcv_op* op);
/* The handle's threshold in MiB (may be fractional; default 128): a tensor at least this large is accessed with streaming hints where
 * a kernel touches it exactly once.  0 switches every hint off.  The binding passes the RCV_STREAM_MIN_MB environment value here once,
 * when it creates the handle; the library itself reads no environment. */
int rcv_set_stream_min_mb(rcv_handle* h, double mb);

/* Label of the kernel (template instantiation / tiling) the library launches for `op`, e.g.
 * "conv_mfma<2,5,4,1,8>" -- written NUL-terminated into buf[0..size). */
int rcv_op_kernel_label(const rcv_handle* h, const rcv_op* op, char* buf, int size);

/* One row of the RCV_OP_PACK job table (device memory, p[RCV_P_IN] -> rcv_pack_job[count]). */
typedef struct rcv_pack_job {
  const float* src;   /* parameter tensor [D0][D1][3][3]                                          */
  float*       dst;   /* [9][rows_pad][cols_pad], zero filled pads                                */
  int32_t D0, D1;
  int32_t rows_from_d1;   /* 1: rows (contraction channel) = d1, cols = d0; 0: rows = d0, cols=d1 */
  int32_t flip;           /* 1: tap t reads source tap 8-t                                        */
  int32_t rows_pad, cols_pad;
  int32_t merged;         /* 1: transposed-conv "merged parity" layout [4 taps (dy,dx)][rows][4*cols] (see conv_mfma.hip);
                           * 2: Winograd layout [16][rows][cols] = G g G^T (see conv_wino.hip);
                           * 3: split-bf16 layout: every value as three bf16 (v = h + m + l exactly); with k = tap * rows_pad + row,
                           *    dst = [plane][k / 32][cols_pad][k % 32] bf16 (k-steps of 32, zero beyond the last tap; rows_pad a multiple of 8,
                           *    of 32 above 32; see conv_bf3.hip / convn_bf3.hip);
                           * 4: layout 1 (merged parity, 4 taps, 4 * cols virtual columns) split the same way (convn_bf3.hip);
                           * 5: split-bf16 in 16-row chunks for the stride-2 wide convs: k = tap * 16 + row % 16 inside chunk row / 16,
                           *    dst = [plane][chunk][5 k-steps][cols_pad][32] bf16 (rows_pad a multiple of 16; conv2_bf3_kernel)      */
  int32_t reserved;
  const float* scale; /* NULL, or one factor per OUTPUT channel (column) applied while packing: inference folds an eval-mode BatchNorm
                       * that follows the conv directly (relu(bn(conv(x))), model.py:175,190-194) into the filter, w'[co] = w[co] * scale[co] */
} rcv_pack_job;

/* One row of the RCV_OP_WGRAD_REDUCE_BATCH job table: the arguments of one RCV_OP_WGRAD_REDUCE record. `first_block` = number of
 * 64-element blocks of the jobs before this one (job j owns blocks [first_block_j, first_block_{j+1}); a block sums 64 consecutive
 * elements of the partial layout [9][CBP][CAP] (+ the bias row): blocks_j = ceil((9*CBP*CAP + (db ? CBP : 0)) / 64), with
 * CAP = CA <= 4 ? 4 : round16(CA), CBP = round16(CB)); i[RCV_I_NPART] of the record = total number of blocks.
 * nsplit == 0: a zero-fill job, db[0..CB) = 0 in ceil(CB / 256) blocks (the RCV_OP_MEMSET of a bias gradient, folded in). */
typedef struct rcv_reduce_job {
  const float* part;  /* [nsplit][9][CBP][CAP] then, if db, [nsplit][CBP]                          */
  float*       dw;    /* [CB][CA][3][3]                                                            */
  float*       db;    /* [CB] or NULL                                                              */
  int32_t nsplit, CB, CA, first_block;
} rcv_reduce_job;

/* One row of the RCV_OP_PRUNE job table (device memory): one weight tensor.  `w` needs 4-byte alignment only (a view into the engine's
 * flat parameter buffer starts anywhere), `mask` none.  The kernel fills `thresh` and `result`; a caller reads the whole table back
 * in one copy. */
typedef struct rcv_prune_job {
  float*   w;          /* n weights, zeroed in place                                                                                 */
  uint8_t* mask;       /* n bytes out: 1 = pruned                                                                                    */
  int64_t  n;
  int64_t  amount;     /* rule 2: how many to zero, 0 <= amount <= n (int(n * r), computed by the host as model.py:649-660)          */
  double   lower, upper;   /* rule 1: the window in per cent                                                                         */
  float    ratio;      /* rule 0                                                                                                     */
  float    thresh;     /* out: the threshold used (rule 2: the selected boundary magnitude, 0 when amount == 0)                      */
  int64_t  result[4];  /* out: { rules 0 / 1: #(|w| < thresh), rule 2: #zeroed by this call; #(w != 0) before; search steps; status } */
} rcv_prune_job;

/* ------------------------------------------------------------------------------------------ */
/* Named entry points (each = fill one record + rcv_run).  Reference call sites they replace:  */
/* ------------------------------------------------------------------------------------------ */

/* nn.Conv2d(k=3,pad=dil,stride,dilation) forward, fused bias / ReLU / BN statistics, optional
 * BatchNorm-apply of the producer folded into the load.   model.py:112,115-116; model.py:170,175
 * Also the data gradient of a stride-1 conv (flipped, transposed filter) and of the transposed
 * conv (aten::convolution_backward under train.py:57).                                          */
int rcv_conv3x3(rcv_handle* h, const rcv_op* op, void* stream);
/* nn.ConvTranspose2d(k=3,s=2,p=1,output_padding=1) forward (model.py:186-187,191) and the data
 * gradient of a stride-2 conv.                                                                  */
int rcv_convT3x3s2(rcv_handle* h, const rcv_op* op, void* stream);
/* filter gradients of both (aten::convolution_backward).                                        */
int rcv_wgrad3x3(rcv_handle* h, const rcv_op* op, void* stream);
/* nn.Conv2d(k=5, pad=2) of the classifiers built with kernelSize / size = 5 (model.py:256-267 Classifier, model.py:403-414
 * UltClassifier; labelPropTrain.py:90-92 builds PB_FCN with kernelSize 5): forward and data gradient (RCV_OP_CONV5).          */
int rcv_conv5x5(rcv_handle* h, const rcv_op* op, void* stream);
/* its filter and bias gradient (RCV_OP_WGRAD5; aten::convolution_backward of model.py:256-267, model.py:403-414).           */
int rcv_wgrad5x5(rcv_handle* h, const rcv_op* op, void* stream);
/* nn.Conv2d(k=1, bias=False) between feature maps (model.py:345 ConvSep.conv_1x1, model.py:366 trConvSep.conv): forward, and with
 * RCV_F_TRANSPOSED_SRC the data gradient (RCV_OP_PW).                                                                       */
int rcv_conv_pw(rcv_handle* h, const rcv_op* op, void* stream);
/* its filter gradient's partial rows (RCV_OP_PW_WGRAD; RCV_OP_PW_WGRAD_REDUCE sums them).                                    */
int rcv_wgrad_pw(rcv_handle* h, const rcv_op* op, void* stream);

/* nn.BatchNorm2d train-mode statistics -> normalisation constants (model.py:113,116,189,192).   *
 *   part [n_part][2][C] -> scale,shift (float[5][C] slot layout c0,c1), mean, istd, running.    */
int rcv_bn_finalize(rcv_handle* h, const float* part, int n_part, int C, double count,
                    const float* gamma, const float* beta, float* running_mean, float* running_var,
                    float momentum, float eps, int training,
                    float* consts /*[5][C]*/, float* save_mean, float* save_istd, void* stream);
/* aten::native_batch_norm_backward reductions -> load constants for RCV_LOAD_GRAD_*.            */
int rcv_bn_backward(rcv_handle* h, const float* part, int n_part, int C, double count,
                    const float* gamma, const float* save_mean, const float* save_istd,
                    const float* fwd_consts, int decoder,
                    float* consts /*[5][C]*/, float* dgamma, float* dbeta, void* stream);

/* nn.MaxPool2d(2,2) of the normalised producer (model.py:97-100).                               */
int rcv_maxpool2x2_fwd(rcv_handle* h, const float* r, const float* consts, float* out,
                       int N, int H, int W, int C, void* stream);

/* CrossEntropyLoss2d (model.py:76-82) + torch.max(pred,1) / pixel accuracy (train.py:70-71).    *
 *   logits NCHW, target int64 [N][H][W]; loss_out[0]=loss, [1]=sum_w, [2]=#correct (as float).  */
int rcv_softmax_ce_argmax_fwd(rcv_handle* h, const float* logits, const int64_t* target,
                              const float* class_weight /*may be NULL*/, int N, int C, int H, int W,
                              float* part, int n_part, float* loss_out, uint8_t* argmax /*may be NULL*/,
                              void* stream);
int rcv_softmax_ce_bwd(rcv_handle* h, const float* logits, const int64_t* target,
                       const float* class_weight, const float* loss_out, const float* grad_out,
                       int N, int C, int H, int W, float* dlogits, void* stream);

/* DiceLoss (model.py:5-43, multi-class branch; train.py:315 --useDice) + arg-max / pixel accuracy.  class_weight is
 * the already rescaled weight vector (model.py:8).  out: float[4 + 16]: [0] = loss, [2] = #correct, [4..] = the
 * per-class coefficients rcv_dice_bwd consumes.                                                                   */
int rcv_dice_fwd(rcv_handle* h, const float* logits, const int64_t* target, const float* class_weight /*may be NULL*/,
                 float eps, int N, int C, int H, int W, float* part, int n_part, float* out,
                 uint8_t* argmax /*may be NULL*/, void* stream);
int rcv_dice_bwd(rcv_handle* h, const float* logits, const int64_t* target, const float* fwd_out, const float* grad_out,
                 int N, int C, int H, int W, float* dlogits, void* stream);

/* train.py:23-27,52-55 (decay * L1 -> gradient decay*sign(p)) + torch.optim.Adam.step            *
 * (train.py:67,357-363) over one flat fp32 buffer; lr is per element group via lr_scale[].      */
/* Per-image confusion matrices from the arg-max mask (uint8) and the labels (int64): replaces the Python
 * mask loops of valid() (train.py:136-153).  counts is int32 [N][C][C] indexed [n][pred][label]; the call ADDS.  A pixel with
 * pred >= C or a label outside [0, C) -- as the int64 it is: -100, 255, 2^32 + c -- is counted nowhere.  Any N >= 1.          */
int rcv_confusion(rcv_handle* h, const uint8_t* argmax, const int64_t* target, int N, int C, int H, int W,
                  int32_t* counts, void* stream);

/* Object-detection precision / recall counts of the reference's validation (getPrecRecall, test.py:28-89,258-262) for every image n and
 * class c in 1..C-1 of pred / target [N][H][W] (uint8 or int64: pred_bytes / target_bytes = 1 or 8; a value outside [1, C) is in no
 * class).  Components are 8-connected and numbered by their first 2x2 block in raster order; each of the K threshold pairs greedily
 * matches the preds, in that order, to the first unused target that passes inter/union > iou_thr[k] (fp64) resp.
 * dist_thr[k] > |centre difference| (centre = bounding-box centre, as cv2.boundingRect).  counts int32 [N][C-1][2+2K] (overwritten):
 * { nPred, nTrue, nCorrIoU[0..K), nCorrDist[0..K) }.  2 <= C <= 8, 1 <= K <= 8, iou_thr[k] finite >= 0, dist_thr[k] finite; the
 * threshold arrays are host memory, read before the call returns.  ws: rcv_op_workspace bytes of the RCV_OP_OBJECT_MATCH record.  */
int rcv_object_match(rcv_handle* h, const void* pred, int pred_bytes, const void* target, int target_bytes, int N, int C, int H, int W,
                     const double* iou_thr, const double* dist_thr, int K, int32_t* counts, void* ws, size_t ws_bytes, void* stream);

/* The objects of a class map, on the device (RCV_OP_OBJECTS): what test.py:43-67 gets from cv2.connectedComponents + cv2.boundingRect + the
 * box centre, with the per-class rules of DBConvert.py:47-102.  classmap [N][H][W] (elem_bytes 1 = uint8, 8 = int64: what predict
 * returns); a pixel is of class v when 1 <= v < C, anything else is background.  Components are 8-connected and numbered per (image,
 * class) by their first 2x2 block in raster order (`rank`, the order of rcv_object_match).  Per class c = 1..C-1 (arrays indexed c-1, HOST
 * memory, read before the call returns): A = components with area > min_area[c] (strict, DBConvert.py:55); amax = the largest area in
 * A (0 if empty); Q = members of A with (double)area >= (double)amax * min_ratio[c] (one fp64 multiply, one compare); Q sorted by area
 * descending, ties by rank ascending; the first min(|Q|, cap[c]) are emitted.  rows int32 [N][C-1][M][8] = { x, y, w, h, area, rank,
 * 2x + w, 2y + h } (x, y, w, h = cv2.boundingRect; the last two = twice the box centre of test.py:59), zero past the emitted count;
 * counts int32 [N][C-1][4] = { components of the class, |A|, |Q|, emitted }.  Every byte of both is written by every call; area is the
 * PIXEL count (not cv2.contourArea).  2 <= C <= 8, 1 <= M <= 16, 0 <= cap[c] <= M, min_area[c] >= 0, min_ratio[c] in [0, 1]; rows and
 * counts 16-byte aligned.  ws: rcv_op_workspace bytes of the RCV_OP_OBJECTS record.  No host synchronisation.                       */
int rcv_find_objects(rcv_handle* h, const void* classmap, int elem_bytes, int N, int C, int H, int W, const int32_t* min_area,
                     const double* min_ratio, const int32_t* cap, int M, int32_t* rows, int32_t* counts, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Object patches on the device (RCV_OP_OBJECT_PATCHES): the step between rcv_find_objects and the patch classifiers (the verifiers of
 * objDetEval.py / classVal.py / classTrainer.py).  frames uint8 [N][Hs][Ws][3]; rows / counts: what rcv_find_objects wrote for N class
 * maps of H x W with C classes and M rows per class (only x, y, w, h of a row and `emitted` of counts are read).  Slot (n, c, k), P =
 * N (C-1) M of them in the order of rows, is valid iff k < min(emitted, M).  For a valid slot:
 *   1. the box in map pixels, every value clamped where it is used (no row content can address outside the frame):
 *      x0 = clamp(x - margin, 0, W - 1), x1 = clamp(x + w + margin, x0 + 1, W); y0, y1 likewise with H;
 *   2. the box in frame pixels, fp64, one correctly rounded division each: fx0 = (x0 Ws) / W, fx1 = (x1 Ws) / W, fy0 = (y0 Hs) / H,
 *      fy1 = (y1 Hs) / H;
 *   3. Pillow's Image.resize((Sw, Sh), BILINEAR, box = (fx0, fy0, fx1, fy1)) of frame n: per axis precompute_coeffs with the box offset
 *      in fp64 (scale = (in1 - in0) / out, support = max(scale, 1), center = in0 + (xx + 0.5) scale, xmin = max(int(center - support +
 *      0.5), 0), xmax = min(int(center + support + 0.5), inSize); triangle weights summed left to right, each divided by the sum, then
 *      int(0.5 + w 2^22)); the horizontal pass first, the vertical pass second, each from 2^21, int32 sums, >> 22, clipped to a byte.
 *      (Pillow itself takes the box as C floats: it agrees byte for byte wherever the four corners are exact in fp32, as they are for
 *      frames of 480 x 640 and maps of 120 x 160; elsewhere this contract is what Pillow computes from the unrounded corners.)
 *   4. step 3 of rcv_rgb_prep: c = byte / 255.0 in fp64, y / u / v rows, products rounded, summed left to right, ((y - 0.5) / 0.5,
 *      u / 0.5, v / 0.5) rounded once to fp32.
 * images float [P][3][Sh][Sw]; bytes uint8 [P][Sh][Sw][3] (the result of step 3) or NULL.  An invalid slot is zero in both; every
 * element of both is written by every call.  1 <= Sh, Sw <= 64, margin >= 0, 1 <= H <= Hs, 1 <= W <= Ws; rows, counts and images
 * 4-byte aligned.  Exact: integers and correctly rounded fp64.  No workspace, no host synchronisation.                           */
int rcv_object_patches(rcv_handle* h, const uint8_t* frames, int N, int Hs, int Ws, const int32_t* rows, const int32_t* counts, int C,
                       int M, int H, int W, int Sh, int Sw, int margin, float* images, uint8_t* bytes /*may be NULL*/, void* stream);

/* Dense optical flow on the device (RCV_OP_FARNEBACK): what transform.py:185-187 optFlow gets from cv2.calcOpticalFlowFarneback(prev,
 * next, None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags), for B frame pairs at once.  prev / next uint8
 * [B][H][W] (channels = 1) or [B][H][W][3] RGB (channels = 3); flow float[B][2][H][W], channel 0 = dx (columns), 1 = dy (rows), the
 * layout optFlow's transpose((2,0,1)) returns: next(x) = prev(x - d) gives +d.  The algorithm is Farnebaeck's (2003) with OpenCV's parameter
 * meanings, stated operation by operation in tests/farneback_restatement.py and DESIGN §4.11 (the project's own contract: agreement with
 * cv2 bit for bit is not claimed).  Refused: flags != 0 (no initial flow, no Gaussian window), pyr_scale != 0.5, even winsize or
 * winsize > 15, poly_n other than 5 or 7, levels > 4.  fp32; every window is summed in a fixed tap order, so the result does not depend
 * on batch position or run.  ws: rcv_op_workspace bytes of the record, 256-byte aligned.  No host synchronisation.                 */
int rcv_farneback_flow(rcv_handle* h, const uint8_t* prev, const uint8_t* next, int channels, int B, int H, int W, float pyr_scale,
                       int levels, int winsize, int iterations, int poly_n, float poly_sigma, int flags, float* flow, void* workspace,
                       size_t workspace_bytes, void* stream);

/* RCV_OP_REMAP_LABELS: what transform.py:189-198 updateLabels gets from cv2.remap(labels, col + flow[0], row + flow[1], INTER_NEAREST,
 * BORDER_CONSTANT, 0) for N class maps (elem_bytes 1 = uint8, 8 = int64) and their flows float[N][2][H][W]: the source pixel is
 * (rint(row + flow[1]), rint(col + flow[0])), sums in fp32, halves to even; 0 where it lies outside the plane (or is NaN).  out must
 * not be labels.                                                                                                                 */
int rcv_update_labels(rcv_handle* h, const void* labels, int elem_bytes, const float* flow, int N, int H, int W, void* out, void* stream);

/* RCV_OP_MAP_FILTER, one launch: N class maps (elem_bytes 1 = uint8, 8 = int64) of num_class = 1..8 classes through a window x window
 * class count (1..15, offsets -(window / 2) ... window - 1 - (window / 2), in-image pixels only) and one rule (RCV_MF_*, defined at the
 * enum): majority vote (labelExtraction.py:70-89: window 4, min_major 15, min_own 7), erosion, and the two halves each of opening and
 * closing (test.py:41's cv2.MORPH_CLOSE is RCV_MF_DILATE_BITS, then RCV_MF_CLOSE_FINISH on its bit map).  set / arg0 / arg1 are i[AUX1] /
 * i[STRIDE] / i[DIL] of the record: (fill_void, min_major, min_own), (S, fill, -), (S, -, -), (S, -, -), (S, fill, -), (S, -, O).
 * in: the class map, for the *_FINISH rules the uint8 bit map; original: the class map of the *_FINISH rules, NULL otherwise; out: the
 * result, never in (uint8 bit map for the *_BITS rules); changed: int32[N] added to, or NULL.  Exact; no workspace, no host
 * synchronisation.                                                                                                              */
int rcv_map_filter(rcv_handle* h, const void* in, const void* original /*may be NULL*/, int elem_bytes, int N, int H, int W, int num_class,
                   int window, int rule, int set, int arg0, int arg1, void* out, int32_t* changed /*may be NULL*/, void* stream);

/* The batch assembly of labelPropTrain.py:162-193 in one launch: for every frame pair b, inputs[2b] = [Ya, Yb, Ya - Yb,
 * labelToPred(label_b)], targets[2b] = label_a, and the swapped sample at 2b + 1; Y = channel 0 of a frame, labelToPred
 * (transform.py:172-183) = -1 everywhere and +1 at the label's class.  images float[B][2][C][H][W], labels int64[B][2][H][W], inputs
 * float[2B][H][W][8] (NHWC: what the network's first conv reads), targets int64[2B][H][W].  num_class must be 5.  A label outside
 * [0, 5) gives -1 in all five class channels (it is never used as an index).  Exact: copies, +-1 and one fp32 subtraction.        */
int rcv_labelprop_batch(rcv_handle* h, const float* images, const int64_t* labels, int B, int C, int H, int W, int num_class,
                        float* inputs, int64_t* targets, void* stream);

/* RCV_OP_LP_INPUT: LabelProp's input for B samples from a prediction of the previous frame, one launch; inputs float[B][H][W][8]
 * (NHWC) = [Ycur, Yprev, Ycur - Yprev, prior], Y = channel 0.  It replaces the loop body of makeLPImages.py:98-100 and the assembly of
 * validLabelProp.py:116-130 run on a class map the network wrote (RCV_OP_CLS_LABEL's uint8 map: prior_bytes 1; int64: 8), and builds the
 * prior the reference leaves commented, `F.softmax(modelSeg(img))*2 - 1.0` (labelPropTrain.py:179,250, validLabelProp.py:118), from fp32
 * NCHW logits float[B][5][H][W] (prior_bytes 4) with the arithmetic stated at RCV_OP_LP_INPUT.  pair = 0: cur float[B][C][H][W], prev
 * float[B][prev_C][H][W] (prev_C = 0: C), prior[s] belongs to sample s.  pair = 1: cur is float[B/2][2][C][H][W] seen as B frames, prev
 * is not read, sample s takes frames s and s ^ 1 and prior[s ^ 1] (labelPropTrain.py:181-182).  plane: float[B][H][W] = Ycur, or NULL.
 * Hard priors are exact (copies, +-1, one fp32 subtraction); num_class must be 5.                                                  */
int rcv_lp_input(rcv_handle* h, const float* cur, const float* prev /*NULL when pair*/, int prev_C, const void* prior, int prior_bytes, int pair,
                 int B, int C, int H, int W, int num_class, float* inputs, float* plane /*may be NULL*/, void* stream);

/* The per-image work of the reference's loader (SSYUVDataset.__getitem__, dataset.py:107-133; ColorJitter, dataset.py:19-39) and the
 * training loop's maskLabel (transform.py:26-49, train.py:43-46) for a whole batch in one launch: frames uint8[B][Hs][Ws][3] (decoded
 * RGB) and labels [B][Hs][Ws] (label_bytes 1 = uint8, 4 = int32: Image.convert('I')) -> imgs float[B][3][H][W] (NCHW: what the network's
 * first conv reads) and targets int64[B][H][W].  Resize = Pillow's 8-bit BILINEAR as two integer passes (horizontal, rounded to uint8,
 * then vertical; out = clip((sum + 2^21) >> 22)) and Pillow's NEAREST index rule for the labels, all from host-made tables:
 * frame_x int32[W][2 + kx] / frame_y int32[H][2 + ky] = {first tap, tap count, 22-bit coefficients} per output index (kx, ky = Pillow's
 * taps per index, ceil(max(in / out, 1)) * 2 + 1 <= 17: an axis shrinks by at most 8; an axis of equal size has the rows {i, 1, 2^22}),
 * label_x int32[W] / label_y int32[H] = source index per output index.  Then norm float[3][256] (to_tensor + Normalize per byte value)
 * and, with train != 0, per image the row params[b] = {flip, b, c, m00, m01, m10, m11, uv_off}: x mirrored when flip != 0,
 * y = (y + b) * c, and unless uv_off != 0 u' = m00 u + m01 v, v' = m10 u + m11 v; train == 0 (the validation loader) takes none of
 * these and params may be NULL.  The label is gathered, mirrored, passed through maskLabel's sequential rule (mask_flags bits 1 = nb,
 * 2 = nr, 4 = ng, 8 = nl) and widened.  Exact (integer passes, a table lookup, two fp32 operations) except u' / v', which are one fused
 * multiply-add each: within 2^-23 (|m0 u| + |m1 v|) of the exact value, as the reference's einsum is.  No random numbers and no
 * trigonometry on the device.                                                                                                    */
int rcv_batch_prep(rcv_handle* h, const uint8_t* frames, const void* labels, int label_bytes, int B, int Hs, int Ws, int H, int W,
                   const int32_t* frame_x, int kx, const int32_t* frame_y, int ky, const int32_t* label_x, const int32_t* label_y,
                   const float* norm, const float* params /*NULL unless train*/, int train, int mask_flags, float* imgs, int64_t* targets,
                   void* stream);

/* RCV_OP_FRAME_PREP: the validation form of rcv_batch_prep for frames alone (the loop of detect.py:125-130 has no labels): imgs are
 * bit for bit what rcv_batch_prep(train = 0) writes for the same frames and tables.                                                */
int rcv_frame_prep(rcv_handle* h, const uint8_t* frames, int B, int Hs, int Ws, int H, int W, const int32_t* frame_x, int kx,
                   const int32_t* frame_y, int ky, const float* norm, float* imgs, void* stream);

/* RCV_OP_RESIZE_U8: the resize stage of rcv_batch_prep alone, for a dataset that is kept on the device.  Pillow's resize ends in a
 * uint8 and everything random (flip, jitter) comes after it, so the bytes can be stored once: frames uint8[B][Hs][Ws][3] -> out
 * uint8[B][H][W][3] (NHWC; the three values rcv_batch_prep looks up in `norm`), labels [B][Hs][Ws] (label_bytes 1 / 4) -> labels_out
 * [B][H][W] of label_out_bytes 1 (uint8; an int32 label keeps its low byte: the caller has checked that every value is <= 255) or 4
 * (int32), gathered through label_x / label_y and not masked.  labels == NULL: frames alone (label_bytes, label_out_bytes, label_x,
 * label_y, labels_out are not looked at).  The tables are rcv_batch_prep's; H == Hs and W == Ws copies.  Exact (integers only).    */
int rcv_resize_u8(rcv_handle* h, const uint8_t* frames, const void* labels /*may be NULL*/, int label_bytes, int B, int Hs, int Ws, int H,
                  int W, const int32_t* frame_x, int kx, const int32_t* frame_y, int ky, const int32_t* label_x, const int32_t* label_y,
                  uint8_t* out, void* labels_out, int label_out_bytes, void* stream);

/* RCV_OP_BATCH_PREP_IDX: rcv_batch_prep whose image b is image index[b] of a store of N images (frames uint8[N][Hs][Ws][3], labels
 * [N][Hs][Ws]); index is int32[B] (index_bytes 4) or int64[B] (8) in device memory, so an epoch's permutation is uploaded once and a
 * batch is a slice of it.  params, imgs, targets have B rows; every other argument is rcv_batch_prep's.  imgs and targets are bit for
 * bit those of rcv_batch_prep on the gathered images.  An index outside [0, N) reads nothing: its image is zeros, its targets 0, and
 * *bad_count (int32, device memory, zeroed by the caller) is incremented once per such image.                                     */
int rcv_batch_prep_indexed(rcv_handle* h, const uint8_t* frames, const void* labels, int label_bytes, int N, const void* index,
                           int index_bytes, int B, int Hs, int Ws, int H, int W, const int32_t* frame_x, int kx, const int32_t* frame_y,
                           int ky, const int32_t* label_x, const int32_t* label_y, const float* norm,
                           const float* params /*NULL unless train*/, int train, int mask_flags, float* imgs, int64_t* targets,
                           int32_t* bad_count, void* stream);

/* RCV_OP_RGB_PREP: the RGB loader of trainer.py:75-123 (SSDataSet with Scale / HorizontalFlip / VerticalFlip / torchvision's PIL
 * ColorJitter / ToYUV / ToTensor / Normalize([.5,0,0],[.5,.5,.5]); the same chain feeds pruner.py, labelPropTrain.py, tester.py,
 * makeLPImages.py, classTrainer.py and objDetEval.py) for a whole batch, on the caller's stream.  frames, labels, the four tables, imgs
 * and targets are rcv_batch_prep's; labels == NULL (then label_bytes = 0, label_x / label_y / targets are not looked at) is the patch
 * chain, which has no label plane.  Per image, in this order:
 *   1. resize: Pillow's 8-bit BILINEAR (frame) / NEAREST (label) from the tables; equal sizes leave the bytes as they are;
 *   2. with train != 0 the row params[b] = {hflip, vflip, n_ops, op0, op1, op2, op3, f_brightness, f_contrast, f_saturation, hue_shift,
 *      0}: x mirrored when hflip != 0, y mirrored when vflip != 0 (frame and label alike), then the first n_ops (0..4) operations in the
 *      row's order on the uint8 RGB pixel, as Pillow computes them (0 = brightness, 1 = contrast, 2 = saturation, 3 = hue; any other code
 *      does nothing).  Image.blend(d, x, f) per byte, fp32 with separately rounded multiply and add: t = d + f (x - d); 0 if t <= 0, 255
 *      if t >= 255, else t truncated.  brightness = blend(0, x, f); contrast = blend(m, x, f), m = floor((2 sum L + n) / (2 n)) over the
 *      n pixels of the image as it stands when the operation runs; saturation = blend(L, x, f); L = (19595 R + 38470 G + 7471 B + 32768)
 *      >> 16.  hue = Pillow's convert("HSV"), H = (H + hue_shift) & 255, convert("RGB"), with every rounding where Pillow has it
 *      (csrc/rgb_prep.hip lists them); the round trip is taken for hue_shift = 0 as well.
 *   3. c = byte / 255.0 in fp64; y, u, v = the rows {0.299, 0.587, 0.114}, {-0.14714119, -0.28886916, 0.43601035}, {0.61497538,
 *      -0.51496512, -0.10001026} times (r, g, b), each product rounded, summed left to right (no fused multiply-add); imgs =
 *      ((y - 0.5) / 0.5, u / 0.5, v / 0.5) rounded once to fp32.
 *   4. label: gather, mirrors, maskLabel (mask_flags as rcv_batch_prep), widened to int64.
 * Contrast depends on the whole image: with stats != 0 a first launch leaves one integer partial sum of L per workgroup in `workspace`
 * (rcv_op_workspace bytes of the record; nothing to zero, no atomics) and the main launch sums its image's partials in a fixed order;
 * stats == 0 promises that no row holds a contrast operation and skips that launch (validation mode takes neither).  Exact: integers,
 * and fp32 / fp64 operations with the roundings above.  No random numbers and no trigonometry on the device.                      */
int rcv_rgb_prep(rcv_handle* h, const uint8_t* frames, const void* labels /*may be NULL*/, int label_bytes, int B, int Hs, int Ws, int H, int W,
                 const int32_t* frame_x, int kx, const int32_t* frame_y, int ky, const int32_t* label_x, const int32_t* label_y,
                 const float* params /*NULL unless train*/, int train, int stats, int mask_flags, float* imgs, int64_t* targets,
                 void* workspace, size_t workspace_bytes, void* stream);

/* RCV_OP_RGB_PREP_IDX: rcv_rgb_prep whose image b is image index[b] of a store of N images (trainer.py:75-123's loader, the store being
 * what Scale leaves: its first transform ends in a uint8 and everything random comes after it).  index is int32[B] (index_bytes 4) or
 * int64[B] (8) in device memory; params, imgs, targets and the partial sums have B rows; every other argument is rcv_rgb_prep's.  imgs
 * and targets are bit for bit those of rcv_rgb_prep on the gathered images.  An index outside [0, N) reads nothing, in either launch:
 * its image is zeros, its targets 0, and *bad_count (int32, device memory, zeroed by the caller) is incremented once per such image. */
int rcv_rgb_prep_indexed(rcv_handle* h, const uint8_t* frames, const void* labels /*may be NULL*/, int label_bytes, int N, const void* index,
                         int index_bytes, int B, int Hs, int Ws, int H, int W, const int32_t* frame_x, int kx, const int32_t* frame_y, int ky,
                         const int32_t* label_x, const int32_t* label_y, const float* params /*NULL unless train*/, int train, int stats,
                         int mask_flags, float* imgs, int64_t* targets, int32_t* bad_count, void* workspace, size_t workspace_bytes,
                         void* stream);

/* RCV_OP_LP_PAIR_PREP: LabelProp's input from a store of N frames at the network's size (frames uint8[N][H][W][3], labels [N][H][W] of
 * label_bytes 1 or 4): the loader of labelPropTrain.py:36-66 for both frames of every pair and the assembly of labelPropTrain.py:162-193
 * in one op.  pairs is int32 / int64 [B][2] in device memory (store indices of frame a and frame b), params float[B][12]: ONE
 * rcv_rgb_prep row per pair.  Both frames and both label planes of pair p take steps 2-4 of rcv_rgb_prep with row p (the same mirrors
 * for all four planes, the same colour operations on both frames, the contrast mean of EACH FRAME ON ITS OWN), no maskLabel; only Y is
 * computed (step 3's fp64 arithmetic, rounded once to fp32).  Then rcv_labelprop_batch: inputs float[2B][H][W][8] (NHWC), sample 2p =
 * {Ya, Yb, Ya - Yb, labelToPred(label_b)}, sample 2p + 1 = {Yb, Ya, Yb - Ya, labelToPred(label_a)}, one fp32 subtraction of the rounded
 * values; a label outside [0, 5) gives -1 in all five class channels; targets int64[2B][H][W] = label_a, label_b.  Bit for bit
 * rcv_labelprop_batch of rcv_rgb_prep of the gathered frames with every row repeated.  num_class must be 5; Hs x Ws must equal H x W
 * (a store at another size is refused when planned).  A pair with either index outside [0, N): both samples zeros, targets 0,
 * *bad_count incremented once.  With train and stats two launches (statistics over the 2B frames, then the main one), else one.   */
int rcv_lp_pair_prep(rcv_handle* h, const uint8_t* frames, const void* labels, int label_bytes, int N, const void* pairs, int pair_bytes, int B,
                     int Hs, int Ws, int H, int W, int num_class, const float* params /*NULL unless train*/, int train, int stats,
                     float* inputs, int64_t* targets, int32_t* bad_count, void* workspace, size_t workspace_bytes, void* stream);

/* RCV_OP_CLS_LABEL, source form 0 without the fused decoder input: labels uint8[N][H][W] = first arg-max over c of
 * (bias[c] + sum_k x[p][k] w[c][k]) (detect.py:131-132), colour uint8[N][H][W][3] = palette[label] (detect.py:133 Colorize) or NULL;
 * x NHWC with CIN = 8 or 16 channels, 1 <= COUT <= 8, palette uint8[8][3] in device memory (NULL iff colour is NULL).               */
int rcv_cls_label(rcv_handle* h, const float* x, const float* w, const float* bias /*may be NULL*/, int N, int H, int W, int CIN, int COUT,
                  uint8_t* labels, uint8_t* colour /*may be NULL*/, const uint8_t* palette, void* stream);
/* RCV_OP_CLS_LABEL, source form 2 (transform.py:158-170 Colorize for a whole batch): colour uint8[N][H][W][3] = palette[classmap], black
 * where the class is outside [0, 8); elem_bytes 1 = uint8, 8 = int64.                                                              */
int rcv_colorize(rcv_handle* h, const void* classmap, int elem_bytes, int N, int H, int W, uint8_t* colour, const uint8_t* palette,
                 void* stream);

/* RCV_OP_CLS_VALID, source form 0 without the fused decoder input: per pixel the first arg-max of (bias[c] + sum_k x[p][k] w[c][k]), the
 * weighted cross-entropy terms against targets int64[N][H][W] (class_weights float[COUT] or NULL) as partial rows float[*n_rows][3] in
 * `workspace` (rcv_op_workspace bytes of the record), counts int32[N][COUT][COUT] += [image][pred][label], labels uint8[N][H][W] or NULL. */
int rcv_cls_valid(rcv_handle* h, const float* x, const float* w, const float* bias /*may be NULL*/, int N, int H, int W, int CIN, int COUT,
                  const int64_t* targets, const float* class_weights /*may be NULL*/, int32_t* counts, uint8_t* labels /*may be NULL*/,
                  void* workspace, size_t workspace_bytes, int* n_rows /*may be NULL*/, void* stream);
/* RCV_OP_VALID_FOLD: state double[76] += this batch (slots at the kind); the loss from `rows` (n_rows > 0, loss NULL) or from the device
 * float `loss` (n_rows = 0, rows NULL); counts are zero afterwards.                                                                   */
int rcv_valid_fold(rcv_handle* h, int32_t* counts, const float* rows, int n_rows, const float* loss, int N, int H, int W, int num_class,
                   double* state, void* stream);
/* RCV_OP_CLS_PROBA, source form 0 without the fused decoder input: softmax over c of (bias[c] + sum_k x[p][k] w[c][k]) with the fixed
 * arithmetic stated at the kind; proba float[N][COUT][H][W], labels uint8[N][H][W], confidence float[N][H][W], pseudo int64[N][H][W]
 * (class where confidence >= threshold, else -100): each may be NULL, not all four.                                                  */
int rcv_cls_proba(rcv_handle* h, const float* x, const float* w, const float* bias /*may be NULL*/, int N, int H, int W, int CIN, int COUT,
                  float* proba, uint8_t* labels, float* confidence, int64_t* pseudo, float threshold, void* stream);
/* RCV_OP_CLS_CALIB, source form 0 without the fused decoder input: class and confidence as rcv_cls_proba forms them, counted into
 * state int64[K + 1][COUT][COUT + 3] (accumulated; layout, bin rule and fixed-point sums at the kind) against targets int64[N][H][W] or
 * NULL and the K ascending edges float[K] in device memory, 1 <= K <= 32.                                                          */
int rcv_cls_calib(rcv_handle* h, const float* x, const float* w, const float* bias /*may be NULL*/, int N, int H, int W, int CIN, int COUT,
                  const int64_t* targets /*may be NULL*/, const float* edges, int K, int64_t* state, void* stream);

/* The BNN-L / BNN-M-C patch classifiers (model.py:569-619; objDetEval.py:89-119, classVal.py).  Each call runs ONE record of the kind
 * named (RCV_OP_BNN_STAGE_FWD / _BWD: conv -> Dropout2d -> MaxPool2d(k, 2) -> ReLU of model.py:590-592,615-618 and its
 * aten::max_pool2d_with_indices_backward / convolution_backward; RCV_OP_BNN_HEAD_FWD / _BWD: fc -> Dropout -> ReLU -> classifier of
 * model.py:593); the slots are documented at the kinds.                                                                          */
int rcv_bnn_stage_fwd(rcv_handle* h, const rcv_op* op, void* stream);
int rcv_bnn_stage_bwd(rcv_handle* h, const rcv_op* op, void* stream);
int rcv_bnn_head_fwd(rcv_handle* h, const rcv_op* op, void* stream);
int rcv_bnn_head_bwd(rcv_handle* h, const rcv_op* op, void* stream);

/* torch.optim.SGD.step (trainer.py:176-178,221): g = grad*grad_scale + weight_decay*p; buf = step==1 ? g : momentum*buf + g;
 * p -= lr*buf.  lr_elem (may be NULL) gives a per-element learning rate (0 = parameter without a gradient: untouched). */
int rcv_sgd_step(rcv_handle* h, float* param, const float* grad, float* momentum_buf, const float* lr_elem /*may be NULL*/,
                 int64_t n, float lr, float momentum, float weight_decay, int step, float grad_scale, void* stream);

/* The same with the prune mask of trainer.py:220-226 / labelPropTrain.py:201-206 / pruner.py:196-202 (`param.grad[indices] = 0` between
 * backward and optimizer.step()): uint8 per element, non-zero = the stored gradient counts as 0, g = weight_decay*p.  The momentum
 * buffer is not masked (a carried-over buffer keeps moving a pruned weight, as under torch.optim.SGD).  As an op record the mask is
 * p[RCV_P_X5], the slot RCV_OP_ADAM_L1 uses.  NULL: bit for bit rcv_sgd_step. */
int rcv_sgd_step_pruned(rcv_handle* h, float* param, const float* grad, float* momentum_buf, const float* lr_elem /*may be NULL*/,
                        const uint8_t* prune_mask /*may be NULL*/, int64_t n, float lr, float momentum, float weight_decay, int step,
                        float grad_scale, void* stream);

/* The mask builders of the reference's prune stage for a whole model in one launch (RCV_OP_PRUNE): pruneModelNew (model.py:45-57, rule
 * RCV_PRUNE_MAX_RATIO), pruneModel (model.py:621-642, RCV_PRUNE_STD_SEARCH) and pruneModel2 (model.py:644-672, RCV_PRUNE_SMALLEST_K) --
 * per tensor two or three `.item()` host syncs in the reference (two per step of pruneModel's search), none here.  `jobs` is DEVICE
 * memory, one row per parameter with dim() > 1; the rows' `thresh` / `result` are outputs (read them back after the stream has run:
 * a status != 0 is that tensor's refusal).  rcv_prune_check validates the same table in HOST memory before it is uploaded and refuses
 * what the reference refuses before it computes anything: amount > n (torch.topk's error), n < 2 under rule 1 (std is NaN), and
 * null / misaligned pointers, n outside [1, 2^31), a ratio or window that is not finite.  Neither call synchronises. */
int rcv_prune_check(const rcv_prune_job* host_jobs, int n_jobs, int rule);
int rcv_prune(rcv_handle* h, rcv_prune_job* jobs, int n_jobs, int rule, void* stream);

/* As an op record, p[RCV_P_IN_AUX] (may be NULL) is a device int32 holding the 1-based step number: it overrides `step` (the
 * bias corrections are then formed on the device), so that a captured graph of the whole training step can be replayed.
 * lr_elem (may be NULL): per-element learning rate; 0 = the element is not stepped at all (a parameter without a gradient).
 * As an op record, p[RCV_P_X5] (may be NULL) is the prune mask of train.py:59-65 (`param.grad[indices] = 0` after backward):
 * uint8 per element of the flat buffer, non-zero = the whole gradient of that element (L1 part included) is zero this step. */
int rcv_adam_l1_step(rcv_handle* h, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                     const float* lr_elem /*may be NULL*/, int64_t n, float lr, float beta1, float beta2,
                     float eps, float decay, int step, float grad_scale, void* stream);
/* the same with the prune mask (rcv_adam_l1_step passes NULL) */
int rcv_adam_l1_step_pruned(rcv_handle* h, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                            const float* lr_elem /*may be NULL*/, const uint8_t* prune_mask /*may be NULL*/, int64_t n, float lr,
                            float beta1, float beta2, float eps, float decay, int step, float grad_scale, void* stream);

/* The same step, which also books the iteration's metrics (train.py:52-53,69-73) in the same launch:
 * metrics[4] (double, device) += { loss_stats[0] + decay*sum|p|, decay*sum|p|, loss_stats[2], 1 } with sum|p| taken before
 * the update (the reference's l1reg(model)); loss_stats = the float row the loss op wrote ([0] loss, [2] #correct pixels).
 * workspace: rcv_op_workspace bytes of an RCV_OP_ADAM_L1 op with the same n (zero-filled once; the launch leaves its ticket
 * zero); workspace_rows = the op's i[RCV_I_NPART].  As an op: p[RCV_P_X3] = metrics, p[RCV_P_X4] = loss_stats, p[RCV_P_PART]. */
int rcv_adam_l1_step_metrics(rcv_handle* h, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                             const float* lr_elem /*may be NULL*/, int64_t n, float lr, float beta1, float beta2,
                             float eps, float decay, int step, float grad_scale, double* metrics, const float* loss_stats,
                             void* workspace, int workspace_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCV_H */
