/*
 * dlwp_hip.h -- C ABI of libdlwp_hip.so: the MI355X (gfx950) forecast-step hot path of DLWP.
 *
 * The reference (jweyn/DLWP) has NO native code and NO FFI: its drop-in boundary is a Python name registry
 * (DLWP/model/models.py:97-103 -> DLWP/util.py:82-93) on top of third-party Keras/TensorFlow ops.  Every entry point
 * below therefore replaces the Keras/TF op(s) that a reference layer resolves to; the reference call site is cited
 * per function.  The Python host layer (dlwp_amd/) binds these with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns int: 0 ok, DLWP_EINVAL (-1) bad argument, DLWP_EUNSUPPORTED (-2), DLWP_EHIP (-3) HIP
 *     runtime error, DLWP_ERCCL (-4) RCCL error; dlwp_last_error() returns a thread-local message for the last non-zero return.
 *   - all tensor pointers are CALLER-OWNED DEVICE memory (e.g. torch-ROCm storage), dense, row-major, NCHW unless
 *     stated; the library never allocates, frees or retains them (rollout objects excepted: buffers captured in a
 *     rollout graph must outlive it).
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it.  No host synchronisation inside.
 *     The Winograd convolutions keep their transformed filters in ONE scratch buffer of the handle (32 MB, allocated at the
 *     first use): launches that share a handle must be ordered on one stream at a time (use one handle per stream
 *     otherwise, or dlwp_conv2d_prepare into caller memory).  A rollout graph prepares into caller memory as well
 *     (dlwp_rollout_workspace_bytes).  Kernel-selection switches live in the handle (dlwp_set_option).
 *   - dtype: the STORAGE type of activation tensors.  DLWP_F32 everywhere; the forward convolutions and
 *     dlwp_maxpool2_fwd also take DLWP_BF16 and, for the convolutions, DLWP_DTYPE_IO(in, out) with different input and
 *     output storage (config 4: bf16 activations between the layers, fp32 state at the model boundary).  Weights, biases
 *     and all arithmetic (MFMA accumulate, activation) are fp32; fp32 -> bf16 rounds to nearest even.
 */
#ifndef DLWP_HIP_H
#define DLWP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLWP_OK            0
#define DLWP_EINVAL       (-1)
#define DLWP_EUNSUPPORTED (-2)
#define DLWP_EHIP         (-3)
#define DLWP_ERCCL        (-4)

#define DLWP_F32  0
#define DLWP_BF16 1
#define DLWP_BF16_O8 2   /* bfloat16 in channel OCTETS: (N, C/8, H, W, 8) -- a pixel's 8 consecutive channels are 16 contiguous
                          * bytes, the unit the bf16 matrix-core kernels stage and multiply.  Only inside DLWP_DTYPE_IO(in, out)
                          * of dlwp_conv2d_fwd / _prepared / dlwp_convlstm_conv_fwd, for layers dlwp_conv2d_supports_dtype
                          * accepts; channel counts and channel windows must be whole octets.  With an O8 OUTPUT,
                          * dlwp_convlstm_conv_fwd reads z_add in octets and keeps the float32 cell state (c_prev, c_out) as
                          * (N, F/8, H, W, 8) float32.  NCHW stays the layout at the model boundary.                        */
#define DLWP_DTYPE_IO(in, out) (0x10000 | (in) | ((out) << 8))   /* input / output storage of one launch */
#define DLWP_DTYPE_IN(d)  (((d) & 0x10000) ? ((d) & 0xff) : (d))
#define DLWP_DTYPE_OUT(d) (((d) & 0x10000) ? (((d) >> 8) & 0xff) : (d))
#define DLWP_COMPUTE_BF16 0x20000   /* OR-ed into a convolution's dtype: a float32-stored INPUT may be rounded to bfloat16
                                     * so that the layer runs on the bf16 matrix cores (config 4's first layers)        */

/* per-axis halo modes */
#define DLWP_PAD_ZERO 0   /* keras.layers.ZeroPadding2D                                  (examples/train.py:163)   */
#define DLWP_PAD_WRAP 1   /* DLWP.custom.PeriodicPadding2D                               (DLWP/custom.py:139-214)  */
#define DLWP_PAD_EDGE 2   /* DLWP.custom.FillPadding2D (pole rows)                       (DLWP/custom.py:309-402)  */
#define DLWP_PAD_REFLECT   3   /* DLWP.custom.TFPadding2D(mode='REFLECT'):   tf.pad mirror WITHOUT the border element  */
#define DLWP_PAD_SYMMETRIC 4   /* DLWP.custom.TFPadding2D(mode='SYMMETRIC'): tf.pad mirror WITH it (custom.py:527-600) */

#define DLWP_ACT_LINEAR 0
#define DLWP_ACT_TANH   1
#define DLWP_ACT_RELU   2

/* how the conv loader reads its stored input tensor */
#define DLWP_SRC_DIRECT    0
#define DLWP_SRC_UPSAMPLE2 1   /* fused keras UpSampling2D(2) in front of the conv       (examples/train.py:191,201) */
#define DLWP_SRC_MAXPOOL2  2   /* fused keras MaxPooling2D(2) in front of the conv       (examples/train.py:171,181) */

typedef struct dlwp_handle* dlwp_handle_t;

typedef struct { int n, c, h, w; } dlwp_shape4;

typedef struct {
  int top, bottom, left, right;   /* asymmetric amounts                                                    */
  int mode_h, mode_w;             /* DLWP_PAD_* per axis; corners follow from applying the two axes in turn */
} dlwp_pad2d;

typedef struct {
  int cout, kh, kw, dil_h, dil_w; /* stride 1, 'valid' after the implicit halo                              */
  dlwp_pad2d halo;                /* fused Periodic/Zero/Fill padding in front of the conv; all-zero = none */
  int act;                        /* DLWP_ACT_* applied in the epilogue after the bias                      */
  int in_c_off, in_c_total;       /* read channels [off, off+xs.c) of a buffer that has in_c_total channels (slice_layer) */
  int out_c_off, out_c_total;     /* write channels [off, off+cout) of a buffer with out_c_total channels (concatenate)   */
  int src_mode;                   /* DLWP_SRC_*: xs describes the STORED tensor; the conv sees it transformed */
  int out_pool;                   /* 1: the epilogue also applies MaxPooling2D(2) -- y is (n, cout, ho/2, wo/2) (forward /
                                   * inference only; ask dlwp_conv2d_supports_out_pool first).  2: 2x2 SUM instead of the
                                   * max (linear activation, no bias; DLWP_EUNSUPPORTED when no kernel instance has it):
                                   * the adjoint of UpSampling2D(2), see dlwp_conv2d_bwd_data_stored                   */
  int out_d2s;                    /* 1: the cout = 4 F channels are the 2x2 PHASES of F fields, phase-major (channel
                                   * (2a + b) F + f = field f at rows 2i + a, columns 2j + b): the epilogue stores them
                                   * interleaved -- y is (n, out_c_total, 2 ho, 2 wo), channels [out_c_off, out_c_off + F) --
                                   * which is dlwp_depth_to_space2 without the pass (inference; ask
                                   * dlwp_conv2d_supports_out_d2s first; not with out_pool)                             */
  int lstm_f, lstm_rec_act;       /* lstm_f = F > 0: this convolution completes the gate pre-activations of a ConvLSTM2D step
                                   * (cout = 4 F, gates i f c o) and its epilogue applies the cell update of
                                   * dlwp_convlstm_gates -- see dlwp_convlstm_conv_fwd, the only entry that takes such a
                                   * descriptor; act = the cell activation, lstm_rec_act = 0 hard_sigmoid | 1 sigmoid; the
                                   * output window (out_c_off, out_c_total) is that of h (F channels).  0: plain Conv2D     */
} dlwp_conv2d;

/* ---- library ---------------------------------------------------------------------------------------------------- */
int         dlwp_version(void);
const char* dlwp_last_error(void);
/* Diagnostics: `text` (NULL: nothing) is written to stdout, followed by a newline, if the process dies of SIGABRT / SIGSEGV / SIGBUS -- the
 * HSA runtime abort()s a process on a GPU memory fault.  bench.py parks its result line here before it runs the one-shot exchange
 * between real GPUs for the first time, and clears it afterwards.  At most 512 KB; earlier handlers are chained.                 */
int         dlwp_set_crash_message(const char* text);
/* One idle wave that occupies `stream`'s hardware queue for `microseconds` (at most 100 000): the probe with which the host layer
 * finds out whether two streams really run beside each other (the runtime multiplexes streams onto a few hardware queues).       */
int         dlwp_spin(dlwp_handle_t h, int microseconds, void* stream);
int         dlwp_create(dlwp_handle_t* h, int device);   /* one handle per device; thread-compatible */
int         dlwp_destroy(dlwp_handle_t h);
int         dlwp_device_info(dlwp_handle_t h, int* cu_count, int* lds_bytes, char* arch, size_t arch_len);
/* Per-handle switches: nothing about kernel selection is process-global, so handles (threads, streams) never see each
 * other's settings.  A new handle starts from the environment (DLWP_WINOGRAD=0, DLWP_BF16_MFMA=0 switch the families off).
 * `previous` (nullable) receives the old value.                                                                       */
#define DLWP_OPT_WINOGRAD           0  /* 3x3 layers with whole channel tiles: Winograd F(2x2,3x3) (1, default) or the direct
                                        * implicit GEMM (0)                                                                */
#define DLWP_OPT_BF16_MFMA          1  /* layers whose INPUT is stored as bf16 (even width, >= 12 channels, no pooling fused
                                        * in): multiply on the bf16 matrix cores with bf16-rounded weights (1, default)     */
#define DLWP_OPT_FORCE_CONV_CONFIG  2  /* tuning sweeps / tests: run this forward tile configuration (-1 = heuristic)      */
#define DLWP_OPT_FORCE_WGRAD_CONFIG 3  /* ... this weight-gradient configuration                                           */
#define DLWP_OPT_WINO_PAIRS         4  /* Winograd on narrow maps (22x45): two samples side by side in one virtual row (1,
                                        * default) or the wide + narrow launch pair (0); same bits either way              */
#define DLWP_OPT_WGRAD_FILL         5  /* weight gradient: how many waves per CU the number of partial-sum splits aims at, in
                                        * eighths of the CU's 16 wave slots (default 4 = half a complement; r2 used 16: measured on
                                        * the six weight gradients of the config-2 U-Net, 8 / 64 samples: 0.306 / 1.291 ms at 16,
                                        * 0.251 / 1.172 ms at 4, 0.263 / 1.820 ms at 2, tools/bench_reduce_jobs.py).  Every
                                        * split writes a slab the size of the weight tensor: fewer splits = less slab traffic    */
#define DLWP_OPT_FEW_STREAM         6  /* 3x3 layers of at most 4 input channels under a pooling epilogue (the first layer):
                                        * the streaming kernel that keeps the weights in registers and walks over the samples
                                        * (csrc/conv_fwd_few.hip) -- 1 (default): from 8 tiles per workgroup on, 0: never,
                                        * 2: whenever the layer qualifies.  Same bits as the direct family's instance.  r4: the
                                        * same switch selects the streaming form of the 16-output-channel Winograd blocks
                                        * (csrc/conv_fwd_wino2s.hip: at most 32 input channels, filters resident in LDS; the
                                        * restated output layer) -- the bits of the position-split instance it stands in for   */
#define DLWP_OPT_SPLITK             7  /* Winograd layers on SMALL grids (a launch under one round of resident workgroups: an
                                        * ensemble share of 1 ... 8 members, 8 training samples per rank): the input channels are
                                        * divided over several workgroups per output tile; the last one to arrive sums the partial
                                        * tiles in index order (deterministic), adds the bias, activates, pools and stores
                                        * (csrc/conv_fwd_k3d1s.hip).  0 (default since r5): never -- a sample's bits do not depend on
                                        * its batch size at all (a member rolls out to the same bits alone, in a
                                        * batch, on 1 GPU or as a shard of 8); the one operating point that gains is 1 ... 2
                                        * members of the 88 x 180 grid (+6 %).  1 (DLWP_SPLITK=1 in the environment):
                                        * by the rule of dlwp_conv2d_split_count; k >= 2: k
                                        * workgroups per tile wherever the layer is eligible (tuning sweeps, tests).  A split
                                        * launch differs from the unsplit one by float32 round-off (another association of the
                                        * same sum); two launches with the SAME split count give the same bits               */
#define DLWP_OPT_WINO_XLOADER       8  /* how the Winograd forward kernel of the 8 x 32 tile fetches its input tile -- bit 0: as
                                        * image-aligned column PAIRS (one 8-byte load per two elements) on float32 plain sources of
                                        * even width under zero / periodic column halos; bit 1: an UP-SAMPLED float32 source at
                                        * source resolution (one load per source element, written to the 2 x 2 tile slots it
                                        * replicates into; zero / periodic / edge halos); bit 2: EDGE PAIRS -- on a map whose
                                        * last 8-row tile is at most half used (44 rows) the blocks of that tile row take the
                                        * valid rows of two neighbouring column tiles each: one block in eighteen less.  7
                                        * (default): all; 0: as before r5 (DLWP_WINO_XLOADER in the environment).  The same
                                        * values reach the same patch positions: identical bits whatever the setting            */
#define DLWP_OPT_WINO_FLAT          9  /* 3x3 float32 Winograd layers of a narrow map (a plain source of at most 46 columns, an
                                        * up-sampled one of at most 46 source columns; 'same' halo of zero / periodic / edge) run
                                        * on runs of 64 consecutive 2x2 tiles instead of 8 x 32 rectangles: no padded tiles
                                        * multiplied (csrc/conv_fwd_wino_flat.hip, launch-info config -4).  0: never; 1 (default):
                                        * from one workgroup per CU on; 2: whenever the layer qualifies.  Not with a forced
                                        * configuration or split-K.  Identical bits whatever the setting (DLWP_WINO_FLAT in the
                                        * environment)                                                                          */
#define DLWP_OPT_FEW_WINO          10  /* the pooled first layer on Winograd multiplies (csrc/conv_fwd_few_wino.hip, launch-info
                                        * config -5): 3x3, dilation 2, at most 4 input channels, whole 32-channel tiles,
                                        * MaxPooling2D(2) epilogue, float32 -- the streaming structure of DLWP_OPT_FEW_STREAM's
                                        * kernel with F(2x2,3x3) on the four parity sub-lattices: 16 multiplies instead of 36.
                                        * 0 (default on every handle): plain dlwp_conv2d_fwd calls keep the direct family's
                                        * bits; 1: a qualifying layer runs the kernel at EVERY batch size (the family follows
                                        * from the geometry alone: a sample's bits do not depend on its batch mates).  The
                                        * bits are those of the general Winograd family on this geometry, i.e. ordinary float32
                                        * round-off away from the direct sum.  Not with a forced configuration.  The inference
                                        * executor of the Python package scopes it to 1 around its own launches and captures
                                        * (DLWP_FEW_WINO=0 in the environment keeps it from doing so)                           */
int         dlwp_set_option(dlwp_handle_t h, int option, int value, int* previous);
/* the defaults themselves: what handles created AFTERWARDS start from, and what the handle-less host logic (planner hints
 * called with a NULL handle, e.g. on a machine without a GPU) uses.  Existing handles are not touched.                 */
int         dlwp_set_default_option(int option, int value, int* previous);

/* ---- halo padding: DLWP.custom.PeriodicPadding2D.call (custom.py:191-214), FillPadding2D.call (custom.py:359-402),
 *      keras ZeroPadding2D.  Generic [outer, H, W, inner] view: NCHW -> outer=N*C, inner=1; NHWC -> outer=N, inner=C.
 *      fwd: y[outer, H+t+b, W+l+r, inner];  bwd: dx = adjoint (halo folded back: wrap adds to the periodic image,
 *      edge adds to the border, zero drops).                                                                          */
int dlwp_pad2d_fwd(dlwp_handle_t, const void* x, void* y, int outer, int h, int w, int inner, dlwp_pad2d p,
                   int dtype, void* stream);
int dlwp_pad2d_bwd(dlwp_handle_t, const void* dy, void* dx, int outer, int h, int w, int inner, dlwp_pad2d p,
                   int dtype, void* stream);

/* ---- keras Conv2D(filters, k, dilation_rate, padding='valid', activation, data_format='channels_first')
 *      (examples/train.py:164-169 ... 214-219) with the halo, UpSampling2D/MaxPooling2D-in-front, bias, activation,
 *      slice_layer (custom.py:675-692) and concatenate fused.  Weights: Keras HWIO (kh,kw,cin,cout); bias (cout).
 *      xs = stored input (n, cin, h, w).  Output (n, cout, ho, wo) with
 *        hin = h (direct) | 2h (upsample2) | h/2 (maxpool2);  ho = hin + top + bottom - dil_h*(kh-1);  same for w.   */
int dlwp_conv2d_out_shape(dlwp_shape4 xs, const dlwp_conv2d* cd, dlwp_shape4* ys);
int dlwp_conv2d_fwd(dlwp_handle_t, const void* x, const void* w, const void* bias, void* y, dlwp_shape4 xs,
                    const dlwp_conv2d* cd, int dtype, void* stream);
/* y AND its MaxPooling2D(2) image y_pool (n, out_c_total, ho/2, wo/2) from one launch: the training forward of a Conv2D under a
 * pooling layer (examples/train.py:164-181: the backward pass needs y, the next layer the pooled tensor).  float32, no other
 * epilogue option in cd; prepared: as dlwp_conv2d_fwd_prepared (built for the same xs / cd with out_pool = 1 -- the instance is
 * chosen as for the pooling epilogue), or NULL.  DLWP_EUNSUPPORTED where the layer's kernel has no such epilogue:
 * dlwp_conv2d_fwd + dlwp_maxpool2_fwd.                                                                                       */
int dlwp_conv2d_fwd_pool2(dlwp_handle_t, const void* x, const void* w, const void* prepared, const void* bias, void* y,
                          void* y_pool, dlwp_shape4 xs, const dlwp_conv2d* cd, int dtype, void* stream);
/* Weight-stationary use (model.predict over many batches, the rollout of DLWP/model/models.py:263-310): some kernel
 * families read the weights in a prepared layout (Winograd G g G^T, packed-N expansion, bf16 arrangement), which
 * dlwp_conv2d_fwd builds in the handle's scratch before every launch (~5 us).  dlwp_conv2d_prepare builds it once into
 * caller-owned device memory of dlwp_conv2d_prepared_bytes() bytes (0: the layer's kernel reads HWIO directly; then
 * `prepared` may be NULL); it is valid for exactly this (xs incl. xs.n, cd, dtype) and until the weights change.        */
size_t dlwp_conv2d_prepared_bytes(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd, int dtype);
int dlwp_conv2d_prepare(dlwp_handle_t, const void* w, void* prepared, dlwp_shape4 xs, const dlwp_conv2d* cd, int dtype,
                        void* stream);
int dlwp_conv2d_fwd_prepared(dlwp_handle_t, const void* x, const void* w, const void* prepared, const void* bias, void* y,
                             dlwp_shape4 xs, const dlwp_conv2d* cd, int dtype, void* stream);
/* same contract, one thread per output element on the vector ALU: any kernel size; used as the in-library cross-check */
int dlwp_conv2d_fwd_direct(dlwp_handle_t, const void* x, const void* w, const void* bias, void* y, dlwp_shape4 xs,
                           const dlwp_conv2d* cd, int dtype, void* stream);

/* tuning hooks (tools/tune_conv.py, tests): enumerate the compiled MFMA tile configurations, ask which one the heuristic
 * picks (-1 = direct kernel); DLWP_OPT_FORCE_CONV_CONFIG forces one.  info9 = {ks, dil, th, tw, waves,
 * frags_per_wave (0: Winograd instance), cout_frags (< 0: packed-N instance for cout <= 16/-cout_frags), channel_chunk,
 * pooled_loader (2: bf16-MFMA instance, only for inputs stored as bf16)}.
 * Not part of the drop-in surface.                                                                                  */
int dlwp_conv2d_num_configs(void);
int dlwp_conv2d_config_info(int i, int* info9, int* lds_bytes);
int dlwp_conv2d_config_flags(int i);        /* bit 0: Winograd instance whose 16-position case splits the positions over two
                                              * waves per tile fragment (conv_fwd_wino2_kernel.h: 2 x waves x 64 threads);
                                              * bit 1: bf16 instance with the ConvLSTM2D cell update in its epilogue
                                              * (dlwp_conv2d.lstm_f; takes only such layers);
                                              * bit 2: position-split instance evaluated in the 32-channel kernel's order of
                                              * operations (same bits as that kernel): for layers with whole 32-channel tiles on
                                              * small grids, where the plain split instances (bit 0 alone) are not offered;
                                              * bit 3 / bit 4: bf16 instance whose input / output is stored in channel octets
                                              * (DLWP_BF16_O8) -- it takes launches with exactly that storage;
                                              * bit 5: Winograd instance with a compiled split-K variant (DLWP_OPT_SPLITK)   */
/* Host logic (no device work; handle nullable = default options): 1 when dlwp_conv2d_fwd(xs, cd, dtype) multiplies with
 * bf16-rounded weights (the bf16-MFMA family), else 0: what a caller comparing against an fp32-weight computation needs to
 * know. */
int dlwp_conv2d_uses_bf16_weights(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd, int dtype);
/* Planner hint (host logic, handle nullable): 1 when a convolution of this geometry behind a MaxPooling2D runs faster with
 * the pooled tensor materialised by dlwp_maxpool2_fwd (the Winograd family has no pooled loader) than with the pooling
 * fused into the direct kernel's loader; 0 otherwise. */
int dlwp_conv2d_prefers_unfused_pool(dlwp_handle_t, int cin, int cout, int kh, int kw, int dil_h, int dil_w);
/* Planner hint (host logic, handle nullable): 1 when a compiled kernel can apply a following MaxPooling2D(2) in the epilogue
 * of this convolution (cd->out_pool = 1): the pre-pooling tensor is then never written. */
int dlwp_conv2d_supports_out_pool(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd);
/* 1 when a compiled matrix-core instance runs this layer with the storage codes of `dtype` (a DLWP_DTYPE_IO value; the question
 * matters for DLWP_BF16_O8, which only the bf16 matrix-core family reads and writes).  Host logic; h may be NULL.            */
int dlwp_conv2d_supports_dtype(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd, int dtype);
/* ... and 1 when a compiled kernel can store the 2x2 phase channels of this convolution interleaved (cd->out_d2s = 1). */
int dlwp_conv2d_supports_out_d2s(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd);
int dlwp_conv2d_pick_config(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd);
/* Measurement hook (bench.py's roofline): what dlwp_conv2d_fwd(xs, cd, dtype) launches -- one kernel, or two when a Winograd
 * layer hands its ragged last column tile to a narrower instance -- and the matrix-core work each launch EXECUTES: the
 * padded GEMM volume its MFMA instructions multiply, 2 FLOP per multiply-add, tile / channel padding included and with
 * Winograd's 16 (9) multiplies per 2x2 outputs instead of the direct 36.  For the fp32 families this is exactly
 * SQ_INSTS_MFMA x 2048 (v_mfma_f32_16x16x4_f32) of a rocprofv3 --pmc pass.  config: index for dlwp_conv2d_config_info
 * (-1: the one-thread-per-output vector kernel, no matrix work; -2 / -3: the streaming kernels of DLWP_OPT_FEW_STREAM -- few
 * input channels under a pooling epilogue / 16-output-channel Winograd blocks --, whose grid is a number of persistent
 * workgroups, not of tiles; -4: the flat Winograd runs of DLWP_OPT_WINO_FLAT; -5: the Winograd first-layer kernel of
 * DLWP_OPT_FEW_WINO).  out2 must hold 2 entries.                                                                   */
typedef struct {
  int config, grid, block_threads;
  double matrix_flops;
  int bf16_matrix;            /* 1: v_mfma_f32_16x16x32_bf16 (peak 2.5 PFLOP/s), 0: fp32 matrix cores (157.3 TFLOP/s) */
  int x_loader;               /* Winograd 8 x 32 instances (DLWP_OPT_WINO_XLOADER): 0 element by element, 1 column pairs, 2 source resolution;
                               * + 4: an edge-pair launch (the last tile row's blocks take two column tiles each)                       */
} dlwp_launch_info;
int dlwp_conv2d_launch_info(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd, int dtype, dlwp_launch_info* out2,
                            int* n_launches);
/* The split regime of dlwp_conv2d_fwd(xs, cd, dtype) on this handle (DLWP_OPT_SPLITK): how many workgroups share the input
 * channels of one output tile -- 1: unsplit.  Two launches of a layer give the same bits for a sample exactly when their split
 * counts are equal (the count follows from the layer and xs.n: every batch size from the chip's first full round of workgroups
 * on is unsplit); across counts the results differ by float32 round-off.                                                     */
int dlwp_conv2d_split_count(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd, int dtype);

/* ---- backward of the fused Conv2D: the two halves of the Keras train step behind DLWPNeuralNet.fit / fit_generator
 *      (DLWP/model/models.py:188-228).  dz = dL/d(pre-activation), (n, out_c_total, ho, wo) window [out_c_off,+cout).
 *      bwd_data : dx = dL/d(input after the src transform, before the halo), (n, cin, hin, win); for DLWP_SRC_DIRECT it
 *                 may be the channel window [in_c_off,+cin) of an in_c_total-channel buffer; for the pooled / up-sampled
 *                 loaders the caller finishes with dlwp_maxpool2_bwd / dlwp_upsample2_bwd.
 *      bwd_weight: dw (kh,kw,cin,cout) HWIO, deterministic (fixed-order slab reduction); accumulate != 0 adds to dw.
 *      Workspace: caller-owned device memory of at least dlwp_conv2d_bwd_workspace(pass 0 = data, 1 = weight) bytes.   */
int dlwp_conv2d_bwd_workspace(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd, int pass, size_t* bytes);
int dlwp_conv2d_bwd_data(dlwp_handle_t, const void* dz, const void* w, void* dx, dlwp_shape4 xs, const dlwp_conv2d* cd,
                         int dtype, void* ws, size_t ws_bytes, void* stream);
/* DLWP_SRC_UPSAMPLE2 layers only: dx = dL/d(STORED tensor), (n, cin, xs.h, xs.w) -- bwd_data followed by
 * dlwp_upsample2_bwd in one kernel (the dense gradient is never written).  DLWP_EUNSUPPORTED when the layer has no kernel
 * instance with the summing epilogue; the caller then takes the two-call route.                                        */
int dlwp_conv2d_bwd_data_stored(dlwp_handle_t, const void* dz, const void* w, void* dx, dlwp_shape4 xs,
                                const dlwp_conv2d* cd, int dtype, void* ws, size_t ws_bytes, void* stream);
int dlwp_conv2d_bwd_weight(dlwp_handle_t, const void* x, const void* dz, void* dw, dlwp_shape4 xs,
                           const dlwp_conv2d* cd, int accumulate, int dtype, void* ws, size_t ws_bytes, void* stream);
/* dlwp_conv2d_bwd_data where the layer's input x is the ACTIVATION OUTPUT of the layer in front (Conv2D -> Conv2D, the decoder of
 * examples/train.py:191-219): dx <- (data gradient) * act'(x) and db_in (xs.c floats, nullable) <- the per-channel sums of that
 * product -- the front layer's dlwp_act_bwd_bias_grad -- from the data gradient's own store phase.  prepared: as
 * dlwp_conv2d_bwd_data_prepared, or NULL (then w is flipped here).  act_in: DLWP_ACT_TANH / RELU.  Workspace:
 * dlwp_conv2d_bwd_workspace(pass = 3).  DLWP_EUNSUPPORTED where the gradient's convolution does not run on the instance with that
 * store phase (8 x 32 Winograd tiles, whole 32-channel tiles of xs.c, plain source, 'same' halo): keep the two calls.            */
int dlwp_conv2d_bwd_data_act(dlwp_handle_t, const void* dz, const void* w, const void* prepared, void* dx, dlwp_shape4 xs,
                             const dlwp_conv2d* cd, const void* x, int act_in, void* db_in, int dtype, void* ws, size_t ws_bytes,
                             void* stream);
/* The weight AND bias gradient of a layer whose only reader is MaxPooling2D(2) and whose data gradient nobody needs (the first
 * layer of the reference's networks, examples/train.py:159-170), from the layer's output y (laid out like dz above) and the
 * POOLED tensor's gradient dpool (n, cout, Ho/2, Wo/2): what dlwp_pool_act_bwd_bias_grad + dlwp_conv2d_bwd_weight compute, without
 * the gradient tensor in between (it is formed in the weight-gradient kernel's loader; ties as dlwp_maxpool2_bwd).  act:
 * DLWP_ACT_LINEAR / TANH / RELU; db nullable.  Workspace: dlwp_conv2d_bwd_workspace(pass = 2).  DLWP_EUNSUPPORTED where no
 * streaming instance fits (3x3, at most 4 input channels): the caller keeps the two calls.                                   */
int dlwp_conv2d_bwd_weight_pooled(dlwp_handle_t, const void* x, const void* y, const void* dpool, void* dw, void* db,
                                  dlwp_shape4 xs, const dlwp_conv2d* cd, int act, int accumulate, int dtype, void* ws,
                                  size_t ws_bytes, void* stream);
int dlwp_conv2d_wgrad_num_configs(void);                                   /* tuning hooks, as for the forward */
int dlwp_conv2d_wgrad_config_info(int i, int* info6, int* lds_bytes);      /* {ks, dil, th, tw, cout_frags (< 0: packed-N
                                                                             * instance for cout <= -cout_frags), waves} */
int dlwp_conv2d_wgrad_config_form(int i, int* cin_block, int* form);      /* input channels per workgroup; form 0 direct, 1
                                                                             * Winograd, 3 channel-block Winograd, 4 the
                                                                             * streaming form for <= 4 input channels */
int dlwp_conv2d_wgrad_pick_config(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd);   /* the heuristic's choice, -1: none */

/* ---- DLWP.custom.RowConnected2D.call / row_conv2d (DLWP/custom.py:825-837, 840-896): a Conv2D whose filters are shared
 *      along a row only -- output row r is the 'valid' convolution of input rows [r, r + kh) with its own kernel w[r]
 *      (custom.py:879-888: one K.conv2d per row slice + concatenate); the optional last layer of the functional U-Net
 *      (examples/train_functional.py:191-196).  The descriptor is dlwp_conv2d with dilation 1, DLWP_SRC_DIRECT -- or, for the
 *      forward and the weight gradient, DLWP_SRC_UPSAMPLE2: the loaders resolve a keras UpSampling2D(2) in front -- and a
 *      plain epilogue (halo, channel windows, bias, activation as for dlwp_conv2d_fwd; output shape: dlwp_conv2d_out_shape).
 *      w: (ho, kh, kw, cin, cout) -- custom.py:800-805; bias: the stored (ho, 1, cout) array of custom.py:812, which
 *      K.bias_add (Keras 2.2, tensorflow backend) reshapes to (1, cout, ho, 1) for channels_first: channel co, row r
 *      receives flat element co * ho + r (nullable).  float32 only; stride 1 (the reference's call sites).
 *      bwd_data : dx (n, cin, h, w) dense <- dL/dx (DLWP_SRC_DIRECT descriptors; behind an up-sampling the caller describes
 *                 the up-sampled tensor and finishes with dlwp_upsample2_bwd); the halo's adjoint is applied through a padded
 *                 temporary of dlwp_rowconv2d_bwd_workspace() bytes (0 without a halo).
 *      bwd_weight: dw (ho, kh, kw, cin, cout) and db (nullable; the stored (ho, 1, cout) layout) from x and dz =
 *                 dL/d(pre-activation), summed over samples and columns in a fixed order (bit-reproducible); accumulate != 0
 *                 adds to dw / db.
 *      _fwd_direct: one thread per output on the vector ALU, the in-library cross-check.
 *      dlwp_rowconv2d_uses_matrix_cores (host logic): 1 when pass 0 = forward | 1 = data | 2 = weight gradient of this
 *      geometry runs on the MFMA kernels, 0 when it takes the vector-ALU route (LDS footprint).                           */
int dlwp_rowconv2d_fwd(dlwp_handle_t, const void* x, const void* w, const void* bias, void* y, dlwp_shape4 xs,
                       const dlwp_conv2d* cd, int dtype, void* stream);
int dlwp_rowconv2d_fwd_direct(dlwp_handle_t, const void* x, const void* w, const void* bias, void* y, dlwp_shape4 xs,
                              const dlwp_conv2d* cd, int dtype, void* stream);
int dlwp_rowconv2d_uses_matrix_cores(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd, int pass);
/* What pass 0 = forward | 1 = data | 2 = weight gradient of this geometry launches (host logic, no stream; the handle may be
 * NULL).  The three entry points above take their launch from the same decision, so this is what runs.  The bias gradient
 * (rowconv2d_bias_grad, cout x ho workgroups behind the weight gradient when db is given) is not part of the report.       */
typedef struct {
  int kind;                 /* 1: the matrix-core kernel instance <targ[0], targ[1]>; 0: the one-thread-per-output vector kernel */
  int targ[2];              /* forward: rowconv2d_fwd_mfma<NSLOT, C4N>; data gradient: rowconv2d_dgrad_mfma<NF> (targ[1] = 0);
                             * weight gradient: rowconv2d_wgrad_mfma<NSLOT, XR>; 0, 0 for the vector kernels                  */
  int grid, block_threads, lds_bytes;   /* grid 0: nothing is launched (forward / data gradient of an empty batch)           */
  int circ;                 /* data gradient: 1 when the periodic column halo is resolved while dz is staged (dx written directly) */
  int fold;                 /* data gradient: 1 when the kernel writes the padded temporary and dlwp_pad2d_bwd follows          */
  int reason;               /* kind 0: 1 kernel taller than the unrolled 5 rows, 2 staged row too wide, 3 LDS footprint, 4 tensor
                             * beyond 32-bit descriptor offsets, 5 empty batch; kind 1: 0                                      */
  int n_cb, n_sg, n_cg, n_mg;   /* kind 1, the grid's factors: column blocks, sample groups, 16-channel groups (cout; data
                                 * gradient: cin fragments / NF), weight gradient M groups of (kx, ci) fragments -- 1 where the
                                 * pass has no such factor (grid = rows x their product; weight gradient: rows x kh x ...)  */
  int samples;              /* kind 1, forward / data gradient: samples per workgroup (S)                                   */
} dlwp_rowconv_launch_info;
int dlwp_rowconv2d_launch_info(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd, int pass, dlwp_rowconv_launch_info* info);
int dlwp_rowconv2d_bwd_workspace(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd, size_t* bytes);
int dlwp_rowconv2d_bwd_data(dlwp_handle_t, const void* dz, const void* w, void* dx, dlwp_shape4 xs, const dlwp_conv2d* cd,
                            int dtype, void* ws, size_t ws_bytes, void* stream);
int dlwp_rowconv2d_bwd_weight(dlwp_handle_t, const void* x, const void* dz, void* dw, void* db, dlwp_shape4 xs,
                              const dlwp_conv2d* cd, int accumulate, int dtype, void* stream);

/* ---- the rest of the train step: Keras 'mse' loss + 'mae' metric (examples/train.py:240, train_functional.py:285),
 *      activation backward, bias gradient, Keras-2.2-form Adam (restated by the reference at DLWP/custom.py:34-40) and
 *      SGD on flat parameter buffers.  Reductions use fixed trees: bit-reproducible.
 *      dlwp_mse_mae: out2[0] = mean((yp-yt)^2), out2[1] = mean(|yp-yt|) (device floats); dy (nullable) =
 *      loss_weight * 2*(yp-yt)/n.  ws >= dlwp_mse_mae_workspace() bytes.                                                */
int    dlwp_act_bwd(dlwp_handle_t, const void* y, const void* dy, void* dz, size_t n, int act, int dtype, void* stream);
size_t dlwp_bias_grad_workspace(int c);
int    dlwp_bias_grad(dlwp_handle_t, const void* dz, void* db, int n, int c, int c_off, int c_total, int hw, void* ws,
                      size_t ws_bytes, int dtype, void* stream);
/* dlwp_act_bwd on channels [c_off, c_off+c) of a (n, c_total, hw) tensor and dlwp_bias_grad of the result in one pass:
 * dz = dy * act'(y) (dz may alias dy), db[c] = sum of dz over (n, hw), by a fixed (bit-reproducible) reduction tree.       */
int    dlwp_act_bwd_bias_grad(dlwp_handle_t, const void* y, const void* dy, void* dz, void* db, int n, int c, int c_off,
                              int c_total, int hw, int act, void* ws, size_t ws_bytes, int dtype, void* stream);
/* dlwp_maxpool2_bwd + dlwp_act_bwd + dlwp_bias_grad in one pass, for a Conv2D whose only reader is MaxPooling2D(2)
 * (DLWP/model/models.py:188-228 train step of the U-Net encoders): y (n,c,h,w) the conv's output, dp (n,c,h/2,w/2) the
 * pooled tensor's gradient, dz (n,c,h,w) <- dL/d(pre-activation), db[c] (nullable) <- sum of dz.  ws as dlwp_bias_grad.  */
int    dlwp_pool_act_bwd_bias_grad(dlwp_handle_t, const void* y, const void* dp, void* dz, void* db, dlwp_shape4 ys, int act,
                                   void* ws, size_t ws_bytes, int dtype, void* stream);
size_t dlwp_mse_mae_workspace(dlwp_handle_t);
int    dlwp_mse_mae(dlwp_handle_t, const void* y_pred, const void* y_true, size_t n, void* out2, void* dy,
                    float loss_weight, void* ws, size_t ws_bytes, int dtype, void* stream);
/* dlwp_mse_mae taken on the PHASE channels of a restated output layer (dlwp_phase_weights: y_phase (n, 4f, h, w), output
 * pixel (2i+a, 2j+b) of field co in channel (2a+b) f + co) against the target y_true (n, f, 2h, 2w): out2 as above;
 * dz_phase (nullable, (n, 4f, h, w)) = what dlwp_space_to_depth2 makes of dy; db4f (nullable, 4f floats) = its sums over
 * (n, h, w), the bias gradient of a linear layer.  One pass instead of dlwp_depth_to_space2 + dlwp_mse_mae +
 * dlwp_space_to_depth2 + dlwp_bias_grad (the train step of examples/train.py's 5x5 output layer, DLWP/model/models.py:188-228). */
size_t dlwp_mse_mae_phase_workspace(int f);
int    dlwp_mse_mae_phase(dlwp_handle_t, const void* y_phase, const void* y_true, int n, int f, int h, int w, void* out2,
                          void* dz_phase, void* db4f, float loss_weight, void* ws, size_t ws_bytes, int dtype, void* stream);
/* the reference's custom losses, on the device (values + gradient, no host round trip):
 *   kind 0: mean((w (yp-yt))^2)                           -- latitude_weighted_loss(mse) (DLWP/custom.py:956-991)
 *   kind 1: regularizer - ACC,  ACC = mean(PT)/sqrt(mean(P^2) mean(T^2)), P = w*yp - mean, T = w*yt - mean
 *           -- anomaly_correlation_loss(mean, regularize_mean, reverse=True) (custom.py:1036-1088), optionally wrapped
 *           in latitude_weighted_loss (examples/train.py:224-234).  regularize: 0 none, 1 'mse', 2 'mae', 3 'global'
 *           (|(mean(T') - mean(P'))/mean(T')| over everything), 4 'spatial' (the same per (sample, channel) plane, averaged),
 *           P' = w*yp, T' = w*yt.
 *   y: (n, c, h, w);  mean: (c, h, w) or null;  row_weights: (h) or null.
 *   stats7 (device) <- {loss, mse, mae, S_pt, S_pp, S_tt, regularizer value};  dy (nullable) <- loss_weight * dL/dyp.   */
size_t dlwp_loss_workspace(dlwp_handle_t, int n, int c);
int    dlwp_loss_custom(dlwp_handle_t, const void* y_pred, const void* y_true, int n, int c, int h, int w,
                        const void* mean, const void* row_weights, int kind, int regularize, void* stats7, void* dy,
                        float loss_weight, void* ws, size_t ws_bytes, int dtype, void* stream);
/* the remaining Keras 2.2 regression losses (keras/losses.py; csrc/losses.hip), x = yp - yt, eps = K.epsilon() = 1e-7, means over
 * all N = n*c*h*w elements; g = d(element value)/d yp, the gradient is g / N:
 *   DLWP_LOSS_MSE      x^2                                                        g = 2x
 *   DLWP_LOSS_MAE      |x|                                                        g = sign(x) (0 at x = 0)
 *   DLWP_LOSS_MAPE     100 |x| / max(|yt|, eps)                                   g = 100 sign(x) / max(|yt|, eps)
 *   DLWP_LOSS_MSLE     (log1p(max(yp, eps)) - log1p(max(yt, eps)))^2             g = 2 (a - b) / (max(yp, eps) + 1), 0 where yp < eps
 *   DLWP_LOSS_LOGCOSH  |x| + log1p(exp(-2|x|)) - log 2  (= x + softplus(-2x) - log 2)   g = tanh(x)
 * dlwp_loss_elementwise: y (n, c, h, w); row_weights (h floats, nullable): the literal latitude weighting loss(w*yt, w*yp) of
 *   DLWP.custom (custom.py:899-991) with w[row] on both operands; out1 (device, 1 float) <- the mean; dy (nullable) <- loss_weight
 *   * dL/dyp = loss_weight * w * g(w yp, w yt) / N.  ws >= dlwp_loss_elementwise_workspace() bytes.
 * dlwp_loss_elementwise_phase: the same on the PHASE channels of a restated output layer (y_phase (n, 4f, h, w) against y_true
 *   (n, f, 2h, 2w), layout as dlwp_mse_mae_phase; w even, y_true 16-byte and the phase tensors 8-byte aligned); dz_phase / db4f (nullable) as there, row
 *   weights indexed by the OUTPUT row.  The bias sums join dlwp_reductions_begin / _flush like dlwp_bias_grad's.
 * dlwp_loss_metrics: one pass over (yp, yt) for the metrics of one output; mask = OR of (1 << DLWP_LOSS_*) and
 *   DLWP_METRIC_ACC_SUMS; out <- the selected means in this order: mse, mae, mape, msle, logcosh, then (ACC sums) mean(yp yt),
 *   mean(yp^2), mean(yt^2).  phase != 0: y_pred is in phase layout and (n, c, h, w) is the target's shape (w % 4 == 0).
 *   ws >= dlwp_loss_metrics_workspace() bytes.
 * Fixed reduction trees, no atomics: bit-reproducible.                                                                      */
#define DLWP_LOSS_MSE     0
#define DLWP_LOSS_MAE     1
#define DLWP_LOSS_MAPE    2
#define DLWP_LOSS_MSLE    3
#define DLWP_LOSS_LOGCOSH 4
#define DLWP_METRIC_ACC_SUMS 0x20u
size_t dlwp_loss_elementwise_workspace(dlwp_handle_t);
int    dlwp_loss_elementwise(dlwp_handle_t, const void* y_pred, const void* y_true, int n, int c, int h, int w,
                             const void* row_weights, int kind, void* out1, void* dy, float loss_weight, void* ws,
                             size_t ws_bytes, int dtype, void* stream);
size_t dlwp_loss_elementwise_phase_workspace(int f);
int    dlwp_loss_elementwise_phase(dlwp_handle_t, const void* y_phase, const void* y_true, int n, int f, int h, int w,
                                   const void* row_weights, int kind, void* out1, void* dz_phase, void* db4f, float loss_weight,
                                   void* ws, size_t ws_bytes, int dtype, void* stream);
size_t dlwp_loss_metrics_workspace(dlwp_handle_t);
int    dlwp_loss_metrics(dlwp_handle_t, const void* y_pred, const void* y_true, int n, int c, int h, int w, int phase,
                         unsigned mask, void* out, void* ws, size_t ws_bytes, int dtype, void* stream);
int    dlwp_adam_keras(dlwp_handle_t, void* p, void* m, void* v, const void* g, size_t n, float lr, float beta_1,
                       float beta_2, float epsilon, float decay, long long iteration, float grad_scale, void* stream);
/* dlwp_adam_keras for a training step captured as a hipGraph: the step number is read from (and advanced in) device memory
 * -- *iteration_dev plays `iteration`, lr_t_scratch is one device float the update reads its step size from.              */
int    dlwp_adam_keras_dev(dlwp_handle_t, void* p, void* m, void* v, const void* g, size_t n, float lr, float beta_1,
                           float beta_2, float epsilon, float decay, long long* iteration_dev, float* lr_t_scratch,
                           float grad_scale, void* stream);
int    dlwp_sgd_keras(dlwp_handle_t, void* p, void* vel, const void* g, size_t n, float lr, float momentum, float decay,
                      long long iteration, float grad_scale, void* stream);
int    dlwp_axpby(dlwp_handle_t, const void* x, void* y, size_t n, float a, float b, void* stream);   /* y = a*x + b*y */
/* ---- the other Keras 2.2.4 optimizers and Keras' gradient clipping (keras/optimizers.py; csrc/optimizers.hip): ONE update entry
 *      with a kind code.  g' below is the gradient the update sees: g * grad_scale, times *factor_dev (nullable: the clipnorm factor
 *      of dlwp_grad_clip_factor), clamped to [-clipvalue, clipvalue] when clipvalue > 0.  it = iteration (the count BEFORE the step),
 *      t = it + 1, lr' = lr / (1 + decay it); step-dependent scalars are evaluated in double on the host and rounded once.
 *        kind              slots        h1, h2        update
 *        SGD               s0 = m       momentum      v = h1 m - lr' g'; m <- v; p += v
 *        SGD_NESTEROV      s0 = m       momentum      v as above; m <- v; p += h1 v - lr' g'
 *        RMSPROP           s0 = a       rho           a <- h1 a + (1 - h1) g'^2; p -= lr' g' / (sqrt(a) + eps)
 *        ADAGRAD           s0 = a                     a <- a + g'^2; p -= lr' g' / (sqrt(a) + eps)
 *        ADADELTA          s0 = a, s1 = d  rho        a as RMSPROP; upd = g' sqrt(d + eps) / sqrt(a + eps); p -= lr' upd;
 *                                                     d <- h1 d + (1 - h1) upd^2
 *        ADAM              s0 = m, s1 = v  b1, b2     dlwp_adam_keras on g'
 *        ADAM_AMSGRAD      + s2 = vhat                vhat <- max(vhat, v); p -= lr_t m / (sqrt(vhat) + eps)
 *        ADAMAX            s0 = m, s1 = u  b1, b2     lr_t = lr' / (1 - b1^t); m as Adam; u <- max(b2 u, |g'|); p -= lr_t m / (u + eps)
 *        NADAM             s0 = m, s1 = v  b1, b2     mu_t = b1 (1 - 0.5 0.96^(t sd)), mu_t1 the same at t + 1 (sd = schedule_decay);
 *                                                     ms_new = m_schedule mu_t, ms_next = ms_new mu_t1 (the CALLER keeps m_schedule:
 *                                                     1 before the first step, ms_new after each); m, v as Adam;
 *                                                     p -= lr ((1 - mu_t) g' / (1 - ms_new) + mu_t1 m / (1 - ms_next))
 *                                                             / (sqrt(v / (1 - b2^t)) + eps);   decay is not used
 *      Unused slot pointers may be null.  One launch; arrays may start at any element of a larger buffer (16-byte accesses where all
 *      of them share their offset inside a 16-byte unit); nothing outside [0, n) is written and g is only read.
 *      dlwp_grad_clip_factor: factor_dev (device, 3 floats) <- {factor, norm, norm^2}, norm = sqrt(sum (g_i grad_scale)^2), factor =
 *      clipnorm / norm where norm >= clipnorm > 0, else exactly 1.  Double-precision fixed tree, no atomics: bit-reproducible.
 *      ws >= dlwp_grad_clip_factor_workspace() bytes, 8-byte aligned.                                                          */
#define DLWP_OPT_SGD           0
#define DLWP_OPT_SGD_NESTEROV  1
#define DLWP_OPT_RMSPROP       2
#define DLWP_OPT_ADAGRAD       3
#define DLWP_OPT_ADADELTA      4
#define DLWP_OPT_ADAM          5
#define DLWP_OPT_ADAM_AMSGRAD  6
#define DLWP_OPT_ADAMAX        7
#define DLWP_OPT_NADAM         8
size_t dlwp_grad_clip_factor_workspace(dlwp_handle_t);
int    dlwp_grad_clip_factor(dlwp_handle_t, const void* g, size_t n, float grad_scale, float clipnorm, void* ws, size_t ws_bytes,
                             float* factor_dev, void* stream);
int    dlwp_optimizer_step(dlwp_handle_t, int kind, void* p, void* s0, void* s1, void* s2, const void* g, size_t n, float lr,
                           float decay, float h1, float h2, float epsilon, float schedule_decay, double m_schedule,
                           long long iteration, float grad_scale, float clipvalue, const float* factor_dev, void* stream);
/* count <= 8 contiguous float32 copies dsts[i] <- srcs[i] (floats[i] elements each) in ONE launch: the batch and its targets
 * on their way into the fixed buffers a captured training step reads (a device-to-device memcpy each before: ~5 us apiece). */
int    dlwp_copy_many(dlwp_handle_t, const void* const* srcs, void* const* dsts, const size_t* floats, int count, void* stream);

/* ---- a training step's weight-side helpers in ONE launch each (csrc/batch.hip).  Keras / TF run one kernel per op
 *      (the train step behind DLWP/model/models.py:188-228); at the 8 samples per GPU of an 8-way data-parallel config-3
 *      step, 32 of 64 launches were sub-5-us helpers on weight-sized tensors.
 *   dlwp_prepare_begin .. dlwp_prepare_flush: dlwp_conv2d_prepare and dlwp_conv2d_bwd_data_prepare in between only RECORD
 *      their work (Winograd filter transforms, packed-N expansions, flipped / transposed kernels); flush builds all of it
 *      with one kernel on `stream`.  (bf16 arrangements are not batched: they run at once.)
 *   dlwp_reductions_begin .. dlwp_reductions_flush: the FINAL sums of dlwp_conv2d_bwd_weight (over its slabs),
 *      dlwp_bias_grad / dlwp_act_bwd_bias_grad / dlwp_pool_act_bwd_bias_grad (over their partials) and dlwp_mse_mae in
 *      between are recorded; their outputs (dw, db, out2) are undefined and their workspaces must stay untouched -- one
 *      workspace per call -- until flush sums everything with one kernel (fixed order: deterministic).  Two recorded sums
 *      into the same tensor (accumulate) flush in between.  At most 24 jobs per launch; more flush early.
 *   The modes live on the handle: one thread per handle while they are on.                                              */
int    dlwp_prepare_begin(dlwp_handle_t);
int    dlwp_prepare_flush(dlwp_handle_t, void* stream);
int    dlwp_reductions_begin(dlwp_handle_t);
int    dlwp_reductions_flush(dlwp_handle_t, void* stream);

/* ---- two INDEPENDENT launches of a training step as ONE kernel launch (r4; csrc/conv_pair.hip).  On grids under one round of
 *      workgroups (8 samples per GPU: every launch of a step) a layer's weight gradient and its data gradient -- both read the
 *      layer's pre-activation gradient, neither reads the other's output -- each leave most CUs idle; issued back to back they cost
 *      the sum of their lifetimes, on two queues more.  Between dlwp_pair_begin and dlwp_pair_end ONE
 *      dlwp_conv2d_bwd_weight and ONE dlwp_conv2d_bwd_data[_stored / _prepared] (in either order) hand their launch over instead of
 *      issuing it; dlwp_pair_end(stream) issues both on `stream` -- as one grid whose first blocks run the weight-gradient
 *      body and whose other blocks run the data-gradient body when a fused instance is compiled for the two kernel
 *      instances (the channel-block Winograd weight gradient on 4 x 32 tiles beside the 8 x 32 Winograd forward instance, 16- or
 *      9-position), one after the other otherwise.  Same bodies, same bits.  The CALLER states the independence; calls the
 *      mode does not cover (another family, a padded-gradient data gradient, a second call of the same kind) run at once.
 *      dlwp_pair_begin on a pair that was never ended (the caller's step raised) issues what that pair holds, launch by launch,
 *      and opens the new one.  dlwp_pair_fused_count: pairs this handle has issued as one launch so far (tests and tools).  */
int    dlwp_pair_begin(dlwp_handle_t);
int    dlwp_pair_end(dlwp_handle_t, void* stream);
long long dlwp_pair_fused_count(dlwp_handle_t);
/* The data gradient's operand -- the flipped / transposed kernel, followed by its Winograd / packed-N form when the
 * gradient's convolution runs on such an instance -- depends on the weights only: build it once per step
 * (dlwp_conv2d_bwd_data_prepare into `prepared`, dlwp_conv2d_bwd_data_prepared_bytes large; batched between
 * dlwp_prepare_begin / _flush) and pass it to dlwp_conv2d_bwd_data_prepared, which then launches the gradient's convolution
 * only.  stored: 0 = dlwp_conv2d_bwd_data semantics, 1 = dlwp_conv2d_bwd_data_stored.  The workspace may be smaller by the
 * kernel's size (kh kw cin cout floats, rounded up to 256 bytes).                                                          */
size_t dlwp_conv2d_bwd_data_prepared_bytes(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd, int stored);
int    dlwp_conv2d_bwd_data_prepare(dlwp_handle_t, const void* w, void* prepared, dlwp_shape4 xs, const dlwp_conv2d* cd,
                                    int stored, void* stream);
int    dlwp_conv2d_bwd_data_prepared(dlwp_handle_t, const void* dz, const void* prepared, void* dx, dlwp_shape4 xs,
                                     const dlwp_conv2d* cd, int dtype, void* ws, size_t ws_bytes, int stored, void* stream);

/* ---- keras MaxPooling2D(2) / UpSampling2D(2) standalone (examples/train.py:171,181,191,201) ------------------------ */
int dlwp_maxpool2_fwd (dlwp_handle_t, const void* x, void* y, dlwp_shape4 xs, int dtype, void* stream);
int dlwp_maxpool2_bwd (dlwp_handle_t, const void* x, const void* dy, void* dx, dlwp_shape4 xs, int dtype, void* stream);
int dlwp_upsample2_fwd(dlwp_handle_t, const void* x, void* y, dlwp_shape4 xs, int dtype, void* stream);
int dlwp_upsample2_bwd(dlwp_handle_t, const void* dy, void* dx, dlwp_shape4 xs, int dtype, void* stream);

/* ---- keras AveragePooling2D(2) standalone: 2x2 / stride 2 / 'valid', x (n, c, h, w) -> y (n, c, h/2, w/2).  A window
 *      a b / c d gives ((a + b) + (c + d)) * 0.25f in float32; with DLWP_BF16 storage the same expression on the widened values,
 *      rounded to nearest-even once at the store.  An odd last row / column belongs to no window.  The backward (DLWP_F32; xs =
 *      shape of dx, dy is (n, c, h/2, w/2)) WRITES every element of dx -- 0.25f * dy inside a window, +0 on an odd last row /
 *      column -- and needs no x.  n == 0 is a no-op; a map of one row or column pools to an empty tensor (y / dy may be null; the
 *      backward still zero-fills dx).  Access width by w and the pointers: w % 4 == 0 with 16-byte aligned x / dx and 8-byte
 *      aligned y / dy: two windows per thread; w even with 8-byte aligned x / dx: one window, 8-byte accesses; else scalar.  All
 *      routes give the same bits.                                                                                              */
int dlwp_avgpool2_fwd (dlwp_handle_t, const void* x, void* y, dlwp_shape4 xs, int dtype, void* stream);   /* DLWP_F32 | DLWP_BF16 */
int dlwp_avgpool2_bwd (dlwp_handle_t, const void* dy, void* dx, dlwp_shape4 xs, int dtype, void* stream); /* DLWP_F32 */

/* ---- keras UpSampling2D(2, interpolation='bilinear') standalone: x (n, c, h, w) -> y (n, c, 2h, 2w), the legacy
 *      tf.image.resize_bilinear scaling (align_corners=False, no half-pixel centres).  In float32, every operation rounded once,
 *      rows first: r[i][2j] = x[i][j] (bits copied), r[i][2j+1] = a + (b - a) * 0.5f with a = x[i][j], b = x[i][min(j+1, w-1)];
 *      then y[2i] = r[i], y[2i+1][s] = t + (u - t) * 0.5f with t = r[i][s], u = r[min(i+1, h-1)][s].  With DLWP_BF16 storage the
 *      same expression on the widened values, rounded to nearest-even once at the store.  The backward (DLWP_F32; xs = shape of
 *      dx, dy is (n, c, 2h, 2w)) is the adjoint in gather form: along one axis g(v)[j] = (v[2j] + 0.5f*v[2j-1]) + 0.5f*v[2j+1],
 *      without the v[2j-1] term at j = 0 and with weight 1 on v[2w-1] at j = w-1; dx = g down the columns of g along the rows of
 *      dy.  It WRITES every element of dx once, without atomics.  n == 0 is a no-op.  Access width by w and the pointers: w even
 *      with 16-byte aligned y / dy and 8-byte aligned x / dx: two source columns per thread; 8-byte aligned y / dy: (even, odd)
 *      pairs; else scalar.  All routes give the same bits.                                                                      */
int dlwp_upsample2_bilinear_fwd(dlwp_handle_t, const void* x, void* y, dlwp_shape4 xs, int dtype, void* stream);   /* DLWP_F32 | DLWP_BF16 */
int dlwp_upsample2_bilinear_bwd(dlwp_handle_t, const void* dy, void* dx, dlwp_shape4 xs, int dtype, void* stream); /* DLWP_F32 */

/* ---- slice_layer (custom.py:675-692) / keras concatenate(axis=1): copy c channels between buffers of different
 *      channel counts.  src (n, src_c_total, h, w) channels [src_off, src_off+c) -> dst channels [dst_off, dst_off+c). */
int dlwp_copy_channels(dlwp_handle_t, const void* src, void* dst, int n, int c, int hw, int src_c_off, int src_c_total,
                       int dst_c_off, int dst_c_total, int dtype, void* stream);

/* ---- predict_timeseries bookkeeping (DLWP/model/models.py:294-300, 448-451): series (T, N, time_dim, V, H*W) ->
 *      (T*time_dim, N, V, H*W).                                                                                        */
int dlwp_series_merge_time(dlwp_handle_t, const void* series, void* out, int t, int n, int time_dim, int v, int hw,
                           int dtype, void* stream);

/* ---- Conv2D on a 2x nearest-neighbour up-sampled tensor, restated on the tensor itself (the decoder layers
 *      UpSampling2D -> padding -> Conv2D of examples/train.py:191-219, Azure/train_tf.py:247-268): the k x k taps fall on few
 *      distinct source pixels, so each of the 4 output phases is a small kernel of summed weights on the low-resolution
 *      tensor; the 4 phases run as ONE convolution with 4*cout channels + a depth-to-space interleave (phase.hip).
 *      dlwp_phase_geometry: per axis, the window [lo, hi] of source offsets and its size k2 for kernel size k and the
 *      top / left halo `pad` of the up-sampled tensor.  dlwp_phase_weights: w (kh,kw,cin,cout), bias -> w2
 *      (kh2,kw2,cin,4*cout), b2 (4*cout, nullable) with column (2a+b)*cout + co for output phase (a, b).                */
int dlwp_phase_geometry(int k, int pad, int* k2, int* lo, int* hi);
int dlwp_phase_weights(dlwp_handle_t, const void* w, const void* bias, void* w2, void* b2, int kh, int kw, int cin, int cout,
                       int pad_top, int pad_left, int dtype, void* stream);
int dlwp_depth_to_space2(dlwp_handle_t, const void* src, void* dst, int n, int f, int h, int w, int c_off, int c_total,
                         int dtype, void* stream);
/* their adjoints, for the training step: dW (+)= the gather of dW2 over the phases (db likewise, nullable pair), and the
 * inverse interleave (n, c_total, 2h, 2w)[c_off:+f] -> (n, 4f, h, w) of a gradient.                                     */
int dlwp_phase_weights_bwd(dlwp_handle_t, const void* dw2, const void* db2, void* dw, void* db, int kh, int kw, int cin,
                           int cout, int pad_top, int pad_left, int accumulate, int dtype, void* stream);
int dlwp_space_to_depth2(dlwp_handle_t, const void* src, void* dst, int n, int f, int h, int w, int c_off, int c_total,
                         int dtype, void* stream);

/* ---- keras Conv2DTranspose(filters, k, strides=2, padding='valid'|'same', data_format='channels_first') (tconv.hip):
 *      y_full[n][o][2i+u][2j+v] += x[n][c][i][j] K[u][v][o][c], K (kh, kw, F, cin), on 2h + max(kh-2, 0) rows; 'same' keeps rows
 *      [pt, pt + 2h), pt = max(kh-2, 0) / 2 (columns alike).  With T = ceil(k / 2) per axis, phase (a, b) of y_full is a stride-1
 *      cross-correlation of x (zero halo T-1 on every side) with w2[ti][tj][c][(2a+b) F + o] = K[a + 2(Th-1-ti)][b + 2(Tw-1-tj)][o][c]
 *      (zero where that index is >= kh / kw): ONE dlwp_conv2d_fwd with 4 F phase-major channels + a cropping interleave.
 *      dlwp_tconv_geometry (host only), per axis: *t = T, *crop = the offset of the output in the interleaved phase tensor
 *      (2 (len + T - 1) long), *out_len = the layer's output length.
 *      dlwp_tconv_weights: K, bias (nullable) -> w2 (sh, sw, cin, 4F), b2 (4F, nullable: the bias once per phase).  sh >= Th and
 *          sw >= Tw taps are stored: the Th x Tw block at offset (oh, ow) = ((sh - Th) / 2, (sw - Tw) / 2), zeros around it (the
 *          matrix-core kernels exist for 3 x 3 and 5 x 5 taps); the convolution's zero halo is then T-1 + oh above / left and
 *          T-1 + (s - T - oh) below / right.  sh = Th, sw = Tw: the map as written above.
 *      dlwp_tconv_weights_bwd: dK[u][v][o][c] (+)= dw2[oh + Th-1-u/2][ow + Tw-1-v/2][c][(2(u&1) + (v&1)) F + o]  (a gather, no sums).
 *      dlwp_depth_to_space2_crop: src (n, 4F, hp, wp) -> dst (n, c_total, out_h, out_w)[c_off:+F],
 *          dst[n][c_off+o][r][s] = src[n][(2((r+top)&1) + ((s+left)&1)) F + o][(r+top)>>1][(s+left)>>1];  top + out_h <= 2 hp,
 *          left + out_w <= 2 wp.
 *      dlwp_space_to_depth2_fill: its adjoint, src (n, c_total, in_h, in_w)[c_off:+F] -> dst (n, 4F, hp, wp): every element of dst
 *          is written, +0 where the crop dropped the pixel.  All float32, bit-exact (they move and zero-fill). */
int dlwp_tconv_geometry(int k, int same, int len, int* t, int* crop, int* out_len);
int dlwp_tconv_weights(dlwp_handle_t, const void* w, const void* bias, void* w2, void* b2, int kh, int kw, int cin, int f,
                       int sh, int sw, int dtype, void* stream);
int dlwp_tconv_weights_bwd(dlwp_handle_t, const void* dw2, void* dw, int kh, int kw, int cin, int f, int sh, int sw,
                           int accumulate, int dtype, void* stream);
int dlwp_depth_to_space2_crop(dlwp_handle_t, const void* src, void* dst, int n, int f, int hp, int wp, int top, int left,
                              int out_h, int out_w, int c_off, int c_total, int dtype, void* stream);
int dlwp_space_to_depth2_fill(dlwp_handle_t, const void* src, void* dst, int n, int f, int hp, int wp, int top, int left,
                              int in_h, int in_w, int c_off, int c_total, int dtype, void* stream);

/* ---- keras Conv2D(filters, k, strides=2, padding='valid'|'same', data_format='channels_first') (sconv.hip):
 *      y[n][o][i][j] = b[o] + sum xpad[n][c][2i+u][2j+v] K[u][v][c][o], K (kh, kw, cin, F).  Per axis -- 'valid': no padding,
 *      out = (len - k) / 2 + 1;  'same' (TensorFlow's rule for stride 2, NOT the stride-1 rule): out = ceil(len / 2),
 *      max((out - 1) 2 + k - len, 0) zeros in all, the smaller half first.  With T = ceil(k / 2) per axis and P the space-to-depth
 *      image of xpad, P[n][(2a+b) cin + c][i][j] = xpad[n][c][2i+a][2j+b] (phase-major, +0 outside the padded image), y is the
 *      stride-1 'valid' cross-correlation of P with w2[ti][tj][(2a+b) cin + c][o] = K[2ti+a][2tj+b][c][o] (zero where that index is
 *      >= kh / kw): ONE dlwp_conv2d_fwd on 4 cin phase-major channels, bias and activation in its epilogue (the bias is the layer's).
 *      dlwp_sconv_geometry (host only), per axis: *t = T, *pad_lo / *pad_hi = the layer's own zero padding, *out_len; an error where
 *          a 'valid' kernel does not fit.
 *      dlwp_sconv_weights: K -> w2 (sh, sw, 4 cin, F).  sh >= Th and sw >= Tw taps are stored: the Th x Tw block at offset (0, 0),
 *          zeros below / right of it (the matrix-core kernels exist for 3 x 3 and 5 x 5 taps); P then has hp = out_h + sh - 1 rows and
 *          wp = out_w + sw - 1 columns, and the convolution stays 'valid' with no halo.
 *      dlwp_sconv_weights_bwd: dK[u][v][c][o] (+)= dw2[u/2][v/2][(2(u&1) + (v&1)) cin + c][o]  (a gather, no sums).
 *      dlwp_space_to_depth2_pad: src (n, c_total, in_h, in_w)[c_off:+c] -> dst (n, 4c, hp, wp),
 *          dst[n][(2a+b) c + ch][i][j] = src[n][c_off+ch][map(2i+a - pad.top, in_h, pad.mode_h)][map(2j+b - pad.left, in_w, pad.mode_w)],
 *          map = the DLWP_PAD_* rule of dlwp_pad2d_fwd; +0 where a map says zero or (2i+a, 2j+b) lies beyond the padded image
 *          (in_h + top + bottom) x (in_w + left + right).  Every element of dst is written.  This is dlwp_pad2d_fwd (the halo layers in
 *          front of the Conv2D and its own 'same' zeros, composed) and the de-interleave in one pass.
 *      dlwp_space_to_depth2_pad_bwd: its adjoint, ddst (n, 4c, hp, wp) -> dsrc (n, c_total, in_h, in_w)[c_off:+c], in gather form (no
 *          atomics): source pixel (y, x) receives the sum of ddst over the padded positions (r, s) inside [0, 2hp) x [0, 2wp) and
 *          inside the padded image that map to it (wrap adds the periodic images, edge adds to the border, the mirrors add their
 *          reflections, zero drops): its own position first, then the halo positions in ascending (r, s).  As dlwp_pad2d_bwd, it
 *          OVERWRITES: every element of the window is written, +0 where nothing maps to it; a caller that already holds a gradient
 *          there adds the result itself.
 *      The four stream entry points refuse, without a launch and in this order: bad sizes / halos / channel windows / stored taps,
 *      null pointers, a null handle.
 *      All float32; all but the sums of the adjoint bit-exact (they move and zero-fill). */
int dlwp_sconv_geometry(int k, int same, int len, int* t, int* pad_lo, int* pad_hi, int* out_len);
int dlwp_sconv_weights(dlwp_handle_t, const void* w, void* w2, int kh, int kw, int cin, int f, int sh, int sw, int dtype,
                       void* stream);
int dlwp_sconv_weights_bwd(dlwp_handle_t, const void* dw2, void* dw, int kh, int kw, int cin, int f, int sh, int sw,
                           int accumulate, int dtype, void* stream);
int dlwp_space_to_depth2_pad(dlwp_handle_t, const void* src, void* dst, int n, int c, int in_h, int in_w, dlwp_pad2d pad, int hp,
                             int wp, int c_off, int c_total, int dtype, void* stream);
int dlwp_space_to_depth2_pad_bwd(dlwp_handle_t, const void* ddst, void* dsrc, int n, int c, int in_h, int in_w, dlwp_pad2d pad,
                                 int hp, int wp, int c_off, int c_total, int dtype, void* stream);

/* ---- keras DepthwiseConv2D / SeparableConv2D (strides 1, data_format='channels_first') (sepconv.hip).  float32 only.
 *      Depthwise stencil, kernel K (kh, kw, cin, dm), bias (cin dm) nullable, output channel c dm + m:
 *          y[n][c dm + m][i][j] = act(b[c dm + m] + sum_{u,v} xpad[n][c][i + u dil_h][j + v dil_w] K[u][v][c][m])
 *      xpad = x under `halo` (the five DLWP_PAD_* modes per axis, the index map of dlwp_pad2d_fwd: the padding layers in front of
 *      the layer and its own 'same' zeros arrive composed); out = padded - dil (k - 1) per axis.  xs = (n, cin, h, w) of the
 *      input WINDOW [in_c_off, +cin) of in_c_total channels; y is window [out_c_off, +cin dm) of out_c_total channels (a total
 *      of 0 = the window itself).  Every output element is one float32 fmaf chain that starts from the bias (or +0) and runs over
 *      the taps in ascending (u, v).
 *      dlwp_depthwise2d_out_shape (host only): ys = (n, cin dm, out_h, out_w), or an error.
 *      dlwp_depthwise2d_bwd_data: the adjoint, halo included, in gather form (no atomics, no workspace):
 *          dx[n][c][y][x] = sum over the padded positions (r, s) that map to (y, x) -- wrap adds the periodic images, edge adds to
 *          the border, the mirrors add their reflections, zero drops: dlwp_pad2d_bwd's semantics -- of
 *          sum_{m,u,v} dz[n][c dm + m][r - u dil_h][s - v dil_w] K[u][v][c][m].
 *          dz lies in the descriptor's OUTPUT window, dx in its input window, which is OVERWRITTEN (every element written).
 *      dlwp_depthwise2d_bwd_weight: dK[u][v][c][m] (+)= sum_{n,i,j} xpad[n][c][i + u dil_h][j + v dil_w] dz[n][c dm + m][i][j].
 *          Two launches: partial sums over fixed runs of 4096 consecutive (n, i, j) positions into ws
 *          (dlwp_depthwise2d_bwd_workspace bytes), then their sum in ascending order; no atomics, the same bits on every run.
 *          accumulate = 1: dK = dK + (that sum), as dlwp_sconv_weights_bwd.
 *      Pointwise product, kernel P (q, o) (= keras (1, 1, q, o)), bias (o) nullable, pixels contiguous:
 *          y[n][o][p] = act(b[o] + sum_q x[n][q][p] P[q][o])             x (n, in_c_total, hw)[in_c_off:+q], y likewise [out_c_off:+o]
 *      on v_mfma_f32_32x32x2_f32: every output element is one q-ordered float32 chain that starts from the bias; a sample's bits do
 *      not depend on the batch it rides in.
 *      dlwp_pointwise2d_bwd_data:   dx[n][q][p] = sum_o dz[n][o][p] P[q][o]   (dz in the output window; dx's window is overwritten)
 *      dlwp_pointwise2d_bwd_weight: dP[q][o] (+)= sum_{n,p} x[n][q][p] dz[n][o][p].  Two launches: partial sums over fixed runs of
 *          16 units (a unit = 32 consecutive pixels of one sample, samples in turn) into ws (dlwp_pointwise2d_bwd_workspace
 *          bytes), then their sum in ascending order; accumulate as above.
 *      act'(y) and the bias gradients are dlwp_act_bwd / dlwp_act_bwd_bias_grad / dlwp_bias_grad on the output.
 *      The stream entry points refuse, without a launch and in this order: bad sizes, halos that do not fit the map, bad channel
 *      windows, null pointers, a null handle. */
typedef struct {
  int kh, kw, dil_h, dil_w;       /* 1 .. 7 taps, dilation 1 .. 4 per axis                                     */
  int depth_multiplier;           /* 1 .. 8                                                                    */
  dlwp_pad2d halo;
  int act;                        /* DLWP_ACT_* after the bias (forward only)                                  */
  int in_c_off, in_c_total;       /* as dlwp_conv2d                                                            */
  int out_c_off, out_c_total;
} dlwp_depthwise2d;
typedef struct {
  int q, o;                       /* input / output channels                                                   */
  int act;                        /* DLWP_ACT_* after the bias (forward only)                                  */
  int in_c_off, in_c_total;
  int out_c_off, out_c_total;
} dlwp_pointwise2d;
int dlwp_depthwise2d_out_shape(dlwp_shape4 xs, dlwp_depthwise2d d, dlwp_shape4* ys);
int dlwp_depthwise2d_fwd(dlwp_handle_t, const void* x, const void* w, const void* bias, void* y, dlwp_shape4 xs, dlwp_depthwise2d d,
                         int dtype, void* stream);
int dlwp_depthwise2d_bwd_data(dlwp_handle_t, const void* dz, const void* w, void* dx, dlwp_shape4 xs, dlwp_depthwise2d d, int dtype,
                              void* stream);
size_t dlwp_depthwise2d_bwd_workspace(dlwp_shape4 xs, dlwp_depthwise2d d);
int dlwp_depthwise2d_bwd_weight(dlwp_handle_t, const void* x, const void* dz, void* dw, dlwp_shape4 xs, dlwp_depthwise2d d, void* ws,
                                int accumulate, int dtype, void* stream);
int dlwp_pointwise2d_fwd(dlwp_handle_t, const void* x, const void* w, const void* bias, void* y, int n, int hw, dlwp_pointwise2d d,
                         int dtype, void* stream);
int dlwp_pointwise2d_bwd_data(dlwp_handle_t, const void* dz, const void* w, void* dx, int n, int hw, dlwp_pointwise2d d, int dtype,
                              void* stream);
size_t dlwp_pointwise2d_bwd_workspace(int n, int hw, dlwp_pointwise2d d);
int dlwp_pointwise2d_bwd_weight(dlwp_handle_t, const void* x, const void* dz, void* dw, int n, int hw, dlwp_pointwise2d d, void* ws,
                                int accumulate, int dtype, void* stream);

/* ---- ConvLSTM2D cell update (keras ConvLSTM2DCell.call; call sites examples/train.py:148-155,
 *      examples/train_functional.py:207-219).  zx / zh: (n, 4F, h*w) gate pre-activations i | f | c | o from the input
 *      convolution (+bias) and the recurrent 'same' convolution of h_{t-1}; zh and c_prev may be NULL on the first step
 *      (h = c = 0).   c = rec(z_f)*c_prev + rec(z_i)*act(z_c);  h = rec(z_o)*act(c).   c_out: dense (n, F, h*w); h is
 *      written to channels [h_c_off, +F) of an h_c_total-channel buffer (the return_sequences output (T*F, h, w)).
 *      act: DLWP_ACT_*; rec_act: 0 = hard_sigmoid (Keras default), 1 = sigmoid.  dtype: DLWP_F32, or
 *      DLWP_DTYPE_IO(z, h) = storage of the gate pre-activations zx / zh and of h (DLWP_F32 | DLWP_BF16 each); the cell
 *      state c and the arithmetic are float32.                                                                        */
/* A ConvLSTM2D step with the cell update in the convolution's epilogue (bfloat16 inference, BASELINE config 4): the 4F gate
 * pre-activations z = conv(x; w) + bias + z_add are NOT stored; the epilogue writes c_out (float32, (n, F, ho, wo)) and h_t
 * (channels [cd->out_c_off, +F) of an out_c_total-channel buffer, storage DLWP_DTYPE_OUT(dtype)).  z_add: the other
 * convolution's stored pre-activations, bfloat16 (n, 4F, ho, wo), or NULL (first step: no recurrent term); c_prev: float32
 * (n, F, ho, wo) or NULL.  cd->lstm_f = F, cd->cout = 4F.  Runs on the bf16 matrix-core instances with 64-channel blocks
 * (4 gates x 16 hidden channels per block): ask dlwp_convlstm_conv_supported first (needs wo % 4 == 0 and a layer the bf16
 * family covers).  prepared: NULL, or the buffer dlwp_conv2d_prepare filled for (xs, cd, dtype).
 * Replaces: one of the two convolutions of a step + dlwp_convlstm_gates (keras ConvLSTM2DCell.call).                      */
int dlwp_convlstm_conv_fwd(dlwp_handle_t, const void* x, const void* w, const void* prepared, const void* bias,
                           const void* z_add, const void* c_prev, void* c_out, void* h_out, dlwp_shape4 xs,
                           const dlwp_conv2d* cd, int dtype, void* stream);
int dlwp_convlstm_conv_supported(dlwp_handle_t, dlwp_shape4 xs, const dlwp_conv2d* cd, int dtype);
/* One ConvLSTM2D step t >= 1 in ONE launch (r3; keras ConvLSTM2DCell.call, the recurrent front end of examples/train.py:144-157):
 * z = conv_h(h_{t-1}) + conv_x(x_t) + bias, then the cell update -- the input convolution's 4 F pre-activations are neither
 * stored nor read back.  cd_h: the recurrent convolution (3x3, 'same' zero halo 1, dilation 1, lstm_f = F <= 24, its channel
 * windows on the h sequence: in = h_{t-1}, out = h_t), xs_h = (n, F, H, W); cd_x: the input convolution (3x3, dilation 2, halo 2
 * of any mode, its channel window on the float32 state), xs_x = (n, Cx <= 8, H, W).  dtype = DLWP_DTYPE_IO(DLWP_BF16_O8,
 * DLWP_BF16_O8): h in octets; c_prev / c_out float32 octets (N, F/8, H, W, 8).  w_h / w_x: the two HWIO kernels (ignored when
 * `prepared` -- dlwp_convlstm_step_prepare's output, dlwp_convlstm_step_prepared_bytes large -- is given); bias: (4 F).       */
int    dlwp_convlstm_step_supported(dlwp_handle_t, dlwp_shape4 xs_h, const dlwp_conv2d* cd_h, dlwp_shape4 xs_x,
                                    const dlwp_conv2d* cd_x, int dtype);
size_t dlwp_convlstm_step_prepared_bytes(dlwp_handle_t, dlwp_shape4 xs_h, const dlwp_conv2d* cd_h, dlwp_shape4 xs_x,
                                         const dlwp_conv2d* cd_x, int dtype);
int    dlwp_convlstm_step_prepare(dlwp_handle_t, const void* w_h, const void* w_x, void* prepared, dlwp_shape4 xs_h,
                                  const dlwp_conv2d* cd_h, dlwp_shape4 xs_x, const dlwp_conv2d* cd_x, int dtype, void* stream);
int    dlwp_convlstm_step_fwd(dlwp_handle_t, const void* h_in, const void* x_in, const void* w_h, const void* w_x,
                              const void* prepared, const void* bias, const void* c_prev, void* c_out, void* h_out,
                              dlwp_shape4 xs_h, const dlwp_conv2d* cd_h, dlwp_shape4 xs_x, const dlwp_conv2d* cd_x, int dtype,
                              void* stream);
int dlwp_convlstm_gates(dlwp_handle_t, const void* zx, const void* zh, const void* c_prev, void* c_out, void* h_out,
                        int n, int f, int hw, int h_c_off, int h_c_total, int act, int rec_act, int dtype, void* stream);
/* backward of the cell update (one step of back-propagation through time behind DLWPNeuralNet.fit on the recurrent
 * model): zx, zh, c_prev as given to the forward, c = the c_out it produced, dh = dL/dh_t read from channels
 * [h_c_off, +F) of an h_c_total-channel gradient buffer, dc_in = dL/dc_t arriving from step t+1 (NULL on the last step).
 * Writes dz (n, 4F, h*w) = dL/d zx = dL/d zh and dc_prev = dL/dc_{t-1} (NULL allowed when there is no previous step). */
int dlwp_convlstm_gates_bwd(dlwp_handle_t, const void* zx, const void* zh, const void* c_prev, const void* c,
                            const void* dh, const void* dc_in, void* dz, void* dc_prev, int n, int f, int hw,
                            int h_c_off, int h_c_total, int act, int rec_act, int dtype, void* stream);

/* ---- keras BatchNormalization(axis=1) on (n, c, hw) float32 tensors: the ('BatchNormalization', None, {'axis': 1}) entry
 *      behind each Conv2D of examples/train.py:170-210, train_generator.py:172-212, Azure/train_tf.py:219-259 (csrc/batchnorm.hip).
 *      Statistics per channel over (n, hw), deterministic (slabs merged with Chan's formula in a fixed order, no atomics).
 *      fwd_train: y = gamma (x - mean_B) / sqrt(var_B + eps) + beta with the batch's biased variance; save_mean / save_invstd
 *                 (c floats) keep mean_B and 1 / sqrt(var_B + eps) for the backward; moving_mean <- m moving_mean +
 *                 (1 - m) mean_B, moving_var <- m moving_var + (1 - m) var_B M / (M - 1), M = n hw > 1, m = momentum.
 *      fwd_infer: the same affine map with the moving statistics (y may alias x).
 *      bwd      : dgamma = sum dy xhat, dbeta = sum dy (both nullable, overwritten), dx (nullable) = gamma invstd
 *                 (dy - (sum dy + xhat sum dy xhat) / M), xhat = (x - save_mean) save_invstd.
 *      gamma / beta nullable (scale=False / center=False: 1 / 0).  Any float alignment.  ws: caller-owned device memory of
 *      dlwp_batchnorm_workspace() bytes, untouched between a call's kernels by anything else.                              */
typedef struct {
  int n, c, hw;                   /* samples, channels, pixels per plane                                  */
  float momentum, epsilon;        /* Keras' momentum (the weight of the OLD moving value) and epsilon      */
} dlwp_batchnorm;
size_t dlwp_batchnorm_workspace(dlwp_batchnorm d);
int dlwp_batchnorm_fwd_train(dlwp_handle_t, const void* x, void* y, const void* gamma, const void* beta, void* moving_mean,
                             void* moving_var, void* save_mean, void* save_invstd, void* ws, size_t ws_bytes, dlwp_batchnorm d,
                             void* stream);
int dlwp_batchnorm_fwd_infer(dlwp_handle_t, const void* x, void* y, const void* gamma, const void* beta,
                             const void* moving_mean, const void* moving_var, dlwp_batchnorm d, void* stream);
int dlwp_batchnorm_bwd(dlwp_handle_t, const void* x, const void* dy, void* dx, const void* gamma, const void* save_mean,
                       const void* save_invstd, void* dgamma, void* dbeta, void* ws, size_t ws_bytes, dlwp_batchnorm d,
                       void* stream);

/* ---- keras Dense and Dropout on float32 row-major matrices: the feed-forward model of examples/train_generator.py:224-233
 *      (Dense(n_features // 2, tanh, l2) -> Dropout(0.25) -> Dense(n_features)) and the dense head of :138-140 (csrc/dense.hip).
 *      x (m, k), w (k, n) = the Keras kernel, b (n) nullable, y / dy (m, n), dx (m, k), dw (k, n), db (n) nullable.
 *      fwd       : y = act(x w + b)
 *      bwd_data  : dx = (dy o act'(y)) w^T                  (y: the forward's output; unused with DLWP_ACT_LINEAR)
 *      bwd_weight: dw = x^T (dy o act'(y)), db = its column sums; both OVERWRITTEN
 *      All products on the float32 matrix instruction, sums in a fixed order, no atomics: two runs give the same bits, and row i
 *      of y / dx does not depend on m or on the other rows.  Any float alignment; no workspace.                              */
typedef struct {
  int m, k, n;                    /* samples, input features, units                                        */
  int act;                        /* DLWP_ACT_*                                                            */
} dlwp_dense;
int dlwp_dense_fwd(dlwp_handle_t, const void* x, const void* w, const void* b, void* y, dlwp_dense d, void* stream);
int dlwp_dense_bwd_data(dlwp_handle_t, const void* dy, const void* y, const void* w, void* dx, dlwp_dense d, void* stream);
int dlwp_dense_bwd_weight(dlwp_handle_t, const void* x, const void* dy, const void* y, void* dw, void* db, dlwp_dense d,
                          void* stream);
/*      Dropout: y[i] = keep(i) ? x[i] * scale : 0 on n contiguous floats (y may alias x).  keep(i) = word (i mod 4) of
 *      Philox-4x32-10 with counter (i / 4 low word, i / 4 high word, step, layer) and key (seed low word, seed high word) is
 *      >= threshold; the caller passes threshold = floor(rate 2^32) and scale = 1 / (1 - rate).  No state: the backward names the
 *      same (seed, layer, step) and multiplies dy by the same mask.  threshold 0, scale 1 is a copy.                          */
typedef struct {
  unsigned long long seed;
  unsigned layer, step;           /* which Dropout layer of the model, which training step                 */
  unsigned threshold;
  float scale;
} dlwp_dropout;
int dlwp_dropout_fwd(dlwp_handle_t, const void* x, void* y, long long n, dlwp_dropout d, void* stream);
int dlwp_dropout_bwd(dlwp_handle_t, const void* dy, void* dx, long long n, dlwp_dropout d, void* stream);

/* ---- keras activation layers (Activation, LeakyReLU, ReLU, ELU, ThresholdedReLU) and merge layers (Add, Subtract, Multiply,
 *      Average, Maximum, Minimum) on n contiguous float32 elements (csrc/eltwise.hip; the closed forms: DESIGN.md section 5.25).
 *      Any float alignment: 16-byte accesses when every operand pointer of a call is 16-byte aligned, element accesses otherwise.
 *      A result never aliases an operand.  No workspace, no atomics: two runs give the same bits.
 *      activation kinds, y = f(x) and dx = dy f'(x) with f' taken from the stored INPUT x; NaN in x gives NaN in y and dx:
 *        DLWP_ELT_RELU          x > theta ? min(x, max_value) : alpha (x - theta)   (alpha 0: 0 for every number x <= theta);
 *                               f' = x > theta ? (x <= max_value ? 1 : 0) : alpha.  alpha >= 0, theta >= 0, max_value > theta
 *                               (+inf: no cap).  LeakyReLU, ReLU, ThresholdedReLU and Activation('relu') are this kind.
 *        DLWP_ELT_ELU           x > 0 ? x : alpha (exp(x) - 1)
 *        DLWP_ELT_SELU          1.0507009873554805 elu(x, 1.6732632423543772)
 *        DLWP_ELT_SIGMOID       1 / (1 + exp(-x));  f' = y (1 - y)
 *        DLWP_ELT_HARD_SIGMOID  clip(0.2 x + 0.5, 0, 1);  f' = 0.2 for -2.5 < x < 2.5, else 0
 *        DLWP_ELT_SOFTPLUS      log(1 + exp(x));  f' = sigmoid(x)
 *        DLWP_ELT_SOFTSIGN      x / (1 + |x|);  f' = 1 / (1 + |x|)^2
 *        DLWP_ELT_TANH          tanh(x), the convolution epilogues' form;  f' = 1 - y^2                                        */
#define DLWP_ELT_RELU         0
#define DLWP_ELT_ELU          1
#define DLWP_ELT_SELU         2
#define DLWP_ELT_SIGMOID      3
#define DLWP_ELT_HARD_SIGMOID 4
#define DLWP_ELT_SOFTPLUS     5
#define DLWP_ELT_SOFTSIGN     6
#define DLWP_ELT_TANH         7
typedef struct {
  int kind;                       /* DLWP_ELT_*                                                            */
  float alpha, max_value, theta;  /* read by DLWP_ELT_RELU (all three) and DLWP_ELT_ELU (alpha)            */
} dlwp_activation;
int dlwp_activation_fwd(dlwp_handle_t, const void* x, void* y, long long n, dlwp_activation d, void* stream);
int dlwp_activation_bwd(dlwp_handle_t, const void* x, const void* dy, void* dx, long long n, dlwp_activation d, void* stream);
/*      merge: y = ((x0 o x1) o x2) o x3 over the first n_src sources (2 to 4; Subtract exactly 2), left to right in float32; the
 *      same tensor may be named as several sources.  Average = that sum / float(n_src), an IEEE division.  Maximum / Minimum
 *      propagate NaN (np.maximum / np.minimum) and keep the LEFT operand of two equal ones.
 *      bwd: every non-null dx_i is OVERWRITTEN in one pass -- Add dy; Subtract dy, -dy; Average dy / float(n_src); Multiply dy
 *      times the product of the other sources multiplied up in source order; Maximum / Minimum dy for the FIRST source equal to
 *      the result and 0 for the others.  The dx_i are distinct tensors, none of them a source or dy.                            */
#define DLWP_MERGE_ADD      0
#define DLWP_MERGE_SUBTRACT 1
#define DLWP_MERGE_MULTIPLY 2
#define DLWP_MERGE_AVERAGE  3
#define DLWP_MERGE_MAXIMUM  4
#define DLWP_MERGE_MINIMUM  5
typedef struct {
  int kind;                       /* DLWP_MERGE_*                                                          */
  int n_src;                      /* sources read: x0 .. x(n_src - 1); the others are ignored              */
} dlwp_merge;
int dlwp_merge_fwd(dlwp_handle_t, const void* x0, const void* x1, const void* x2, const void* x3, void* y, long long n,
                   dlwp_merge d, void* stream);
int dlwp_merge_bwd(dlwp_handle_t, const void* x0, const void* x1, const void* x2, const void* x3, const void* dy, void* dx0,
                   void* dx1, void* dx2, void* dx3, long long n, dlwp_merge d, void* stream);

/* ---- the wrapper's scaler and imputer on the device: DLWPNeuralNet(scaler_type='StandardScaler' | 'MinMaxScaler',
 *      impute_missing=True) runs SimpleImputer.transform and the scaler's transform in front of every model call and the
 *      scaler's inverse_transform behind it (DLWP/model/models.py:134-170, 230-245) -- sklearn on the host.  Here one launch per
 *      direction on n samples of f contiguous float32 features (csrc/scale.hip).  fill / shift / scale: per-feature FLOAT64
 *      device arrays of f elements (sklearn's statistics_, mean_ | min_, scale_), each nullable = that stage is left out
 *      (no imputer, with_mean=False, with_std=False).  The arithmetic is numpy's when sklearn updates a float32 array in place
 *      with float64 parameters -- every stage in double, rounded to float32 BEFORE the next one, IEEE division, no fused
 *      multiply-add -- so the results equal sklearn's bit for bit:
 *          fwd, impute                : x = isnan(x) ? (float)fill[j] : x
 *          fwd, DLWP_SCALE_STANDARD   : t = (float)((double)x - shift[j]);  y = (float)((double)t / scale[j])
 *          fwd, DLWP_SCALE_MINMAX     : t = (float)((double)x * scale[j]);  y = (float)((double)t + shift[j])
 *          inv, DLWP_SCALE_STANDARD   : t = (float)((double)x * scale[j]);  y = (float)((double)t + shift[j])
 *          inv, DLWP_SCALE_MINMAX     : t = (float)((double)x - shift[j]);  y = (float)((double)t / scale[j])
 *      y may alias x.  float4 accesses where f % 4 == 0 and x, y are 16-byte aligned, element accesses otherwise (any float
 *      alignment).  Inference only: never part of a recorded training step.                                                  */
#define DLWP_SCALE_STANDARD 0
#define DLWP_SCALE_MINMAX   1
typedef struct {
  int n, f;                       /* samples, features per sample                                          */
  int kind;                       /* DLWP_SCALE_*                                                          */
} dlwp_scale;
int dlwp_scale_fwd(dlwp_handle_t, const void* x, void* y, const void* fill, const void* shift, const void* scale, dlwp_scale d,
                   void* stream);
int dlwp_scale_inv(dlwp_handle_t, const void* x, void* y, const void* shift, const void* scale, dlwp_scale d, void* stream);

/* ---- rollout: the N-step predict_timeseries loop (DLWP/model/models.py:277-293, 439-447) captured as ONE hipGraph.
 *      A plan is an array of dlwp_op describing one model call; buffer index >= 0 = caller scratch buffer,
 *      DLWP_BUF_STATE_IN = the call's input state, DLWP_BUF_OUT(o) = output o of the call.  Call t reads
 *      state0 (t == 0) or slot t*n_outputs-1 of `series` and writes slots [t*n_outputs, (t+1)*n_outputs).          */
#define DLWP_BUF_STATE_IN (-1)
#define DLWP_BUF_OUT(o)   (-2 - (o))
#define DLWP_OP_CONV2D     0
#define DLWP_OP_PAD2D      1
#define DLWP_OP_MAXPOOL2   2
#define DLWP_OP_UPSAMPLE2  3
#define DLWP_OP_COPYCH     4
#define DLWP_OP_LSTM_GATES 5
#define DLWP_OP_PHASE_WEIGHTS 6   /* src = kernel buffer, w = -1 | bias buffer index in b, dst = w2 buffer, aux[0] = b2 buffer |
                                   * -1000; conv = {cout, kh, kw, halo.top, halo.left}, xs.c = cin.  Run ONCE at the head of
                                   * the rollout graph (the weights do not change inside a launch). */
#define DLWP_OP_DEPTH2SPACE 7     /* src (n, 4F, h, w) -> dst window [conv.out_c_off, +F) of conv.out_c_total channels at
                                   * (2h, 2w); xs = (n, F, h, w) */
#define DLWP_OP_ROWCONV2D  8      /* dlwp_rowconv2d_fwd: src, dst, w, b, xs, conv as for DLWP_OP_CONV2D (float32 buffers) */
#define DLWP_OP_BATCHNORM  9      /* dlwp_batchnorm_fwd_infer: src, dst, xs = (n, c, h, w); w / b = gamma / beta buffer | -1,
                                   * aux[0] / aux[1] = moving mean / variance buffer, aux[2] = the bits of epsilon (float).
                                   * The moving statistics are read at every launch: a graph never holds stale ones.      */
#define DLWP_OP_DENSE     10      /* dlwp_dense_fwd: src, dst, w, b (| -1); xs = (n, k, 1, 1), conv.cout = units, conv.act       */
#define DLWP_OP_SCALE     11      /* dlwp_scale_fwd / dlwp_scale_inv: src, dst (may be the same buffer), xs = (n, c, h, w) with
                                   * f = c h w; w / b = shift / scale buffer | -1, aux[0] = fill buffer | -1000, aux[1] =
                                   * DLWP_SCALE_*, aux[2] = 0 forward | 1 inverse (no fill).  float64 parameter buffers, read
                                   * at every launch: a graph never holds a refitted scaler's old values.                  */
#define DLWP_OP_ACTIVATION 12     /* dlwp_activation_fwd: src, dst, xs = (n, c, h, w) with n c h w elements; conv.act = DLWP_ELT_*,
                                   * aux[0..2] = the bits of alpha, max_value, theta (floats)                               */
#define DLWP_OP_MERGE     13      /* dlwp_merge_fwd: src = the first source, aux[0..2] = the others | -1000, dst, xs as above;
                                   * conv.act = DLWP_MERGE_*                                                                */
#define DLWP_OP_AVGPOOL2  14      /* dlwp_avgpool2_fwd: src, dst, xs = (n, c, h, w) of src; aux[0] = storage dtype of both tensors */
#define DLWP_OP_BILINEAR2 15      /* dlwp_upsample2_bilinear_fwd: src, dst, xs = (n, c, h, w) of src; aux[0] = storage dtype of both tensors */
#define DLWP_OP_TCONV_WEIGHTS 16  /* dlwp_tconv_weights: buffers as for DLWP_OP_PHASE_WEIGHTS (aux[0] = b2 | -1000); conv = {cout = F,
                                   * kh, kw}, xs.c = cin, aux[1] / aux[2] = sh / sw.  Run ONCE at the head of the rollout graph. */
#define DLWP_OP_DEPTH2SPACE_CROP 17 /* dlwp_depth_to_space2_crop: src (n, 4F, hp, wp) -> dst window [conv.out_c_off, +F) of
                                   * conv.out_c_total channels; xs = (n, F, hp, wp), aux = {top, left, out_h, out_w} */
#define DLWP_OP_CROP2D    18      /* keras Cropping2D = dlwp_pad2d_bwd with DLWP_PAD_ZERO: src (n, c, h, w) -> dst (n, c, h - top -
                                   * bottom, w - left - right); xs = (n, c, h, w) of src, pad = the cropping */
#define DLWP_OP_SCONV_WEIGHTS 19  /* dlwp_sconv_weights: src = the layer's kernel, dst = w2 (parameter buffers); conv = {cout = F, kh,
                                   * kw}, xs.c = cin, aux[1] / aux[2] = sh / sw.  Run ONCE at the head of the rollout graph.   */
#define DLWP_OP_SPACE2DEPTH_PAD 20 /* dlwp_space_to_depth2_pad: src window [conv.in_c_off, +xs.c) of conv.in_c_total channels, xs =
                                   * (n, c, h, w) of that window -> dst (n, 4c, hp, wp); pad = the halo, aux = {hp, wp}        */
#define DLWP_OP_DEPTHWISE2D 21    /* dlwp_depthwise2d_fwd: xs = (n, cin, h, w) of the input window; conv = {kh, kw, dil, halo, act, the
                                   * channel windows}, aux[0] = depth_multiplier; w / b = depthwise kernel / bias (b may be NONE)  */
#define DLWP_OP_POINTWISE2D 22    /* dlwp_pointwise2d_fwd: xs = (n, q, h, w); conv = {cout = o, act, the channel windows}; w / b  */
typedef struct {
  int kind;                 /* DLWP_OP_*                                                                */
  int src, dst;             /* buffer indices                                                              */
  int w, b;                 /* weight / bias buffer indices (conv only)                                    */
  dlwp_shape4 xs;           /* stored input shape of this op                                               */
  dlwp_conv2d conv;         /* DLWP_OP_CONV2D; for DLWP_OP_COPYCH: in_c_off/in_c_total/out_c_off/out_c_total */
  dlwp_pad2d pad;           /* DLWP_OP_PAD2D (NHWC: xs = (n,1,h,w) and conv.in_c_total = channels)          */
  int aux[4];               /* DLWP_OP_LSTM_GATES: src = zx, dst = h buffer (window conv.out_c_off/out_c_total), xs =
                             * (n, F, h, w), aux = {zh | -1000, c_prev | -1000, c_out, rec_act + 256 * (h buffer stored as
                             * bfloat16) + 512 * (zx / zh stored as bfloat16)}, conv.act = activation.
                             * DLWP_OP_CONV2D / DLWP_OP_MAXPOOL2 / DLWP_OP_AVGPOOL2 / DLWP_OP_BILINEAR2: aux[0] = storage dtype of this op's tensors (DLWP_F32,
                             * DLWP_BF16 or DLWP_DTYPE_IO(in, out)); the rollout's own dtype describes state and series.
                             * DLWP_OP_CONV2D with conv.lstm_f > 0 (dlwp_convlstm_conv_fwd): dst = h buffer, aux[1..3] =
                             * {z_add | -1000, c_prev | -1000, c_out}                                                  */
  /* DLWP_OP_CONV2D with conv.lstm_f > 0 and src2 != -1000: a whole ConvLSTM2D step (dlwp_convlstm_step_fwd) -- conv = the
   * recurrent convolution, src = dst = the h buffer, w / b = recurrent kernel / the layer's bias; src2 = the float32 state the
   * input convolution conv2 reads xs2_c channels of, w2 = its kernel.  Every other op: src2 = -1000.                       */
  int src2, w2, xs2_c;
  dlwp_conv2d conv2;
} dlwp_op;
#define DLWP_BUF_NONE (-1000)
typedef struct dlwp_rollout* dlwp_rollout_t;
/* workspace: caller-owned device memory of dlwp_rollout_workspace_bytes() bytes that must outlive the rollout -- the
 * prepared weights of the Winograd / packed-N / bf16 layers live there, rebuilt by the first kernels of every launch (the
 * weights may change between launches).  The library allocates no device memory for a rollout.                        */
size_t dlwp_rollout_workspace_bytes(dlwp_handle_t, const dlwp_op* plan, int n_ops, int groups);
int dlwp_rollout_create(dlwp_handle_t, const dlwp_op* plan, int n_ops, void* const* buffers, int n_buffers,
                        const void* state0, void* series, size_t slot_elems, int calls, int n_outputs, int dtype,
                        void* workspace, size_t workspace_bytes, dlwp_rollout_t* out);
/* The same with the members (xs.n of the ops) split into `groups` equal parts captured as parallel graph branches:
 * members are independent, so an ensemble can run as several chains whose kernels fill the gaps each other's launches
 * leave.  buffer_sample_bytes[i] = bytes ONE member occupies in scratch buffer i (0 for weight / bias buffers); the member
 * count must be a multiple of groups.  groups = 1 is dlwp_rollout_create.                                               */
int dlwp_rollout_create_grouped(dlwp_handle_t, const dlwp_op* plan, int n_ops, void* const* buffers, int n_buffers,
                                const size_t* buffer_sample_bytes, int groups, const void* state0, void* series,
                                size_t slot_elems, int calls, int n_outputs, int dtype, void* workspace,
                                size_t workspace_bytes, dlwp_rollout_t* out);
/* `dtype` of the two create calls may carry DLWP_ROLLOUT_PREPARED: the graph is a later TIME SLICE of a rollout (state0 = the
 * previous slice's last series slot) that shares `workspace` with the first slice and is always launched behind it on the same
 * stream -- it does not prepare the weights again.                                                                          */
#define DLWP_ROLLOUT_PREPARED 0x100
/* ---- a rollout whose model outputs are NOT its next inputs: TimeSeriesEstimator.predict (DLWP/model/extensions.py:206-240, the
 *      forecast examples/validate.py:191-205 runs: inputs = 2 time steps x (variables + insolation), outputs = 2 x variables) and
 *      the step_sequence branch of DLWPNeuralNet.predict_timeseries (DLWP/model/models.py:280-290).  Between two model calls the
 *      reference rebuilds the input on the host (reindex of the sample axis by k, impute, insolation of the rows past the data,
 *      .loc assignment of the predicted channels); dlwp_state_feedback is that update as ONE launch on device-resident tensors:
 *      for every row i < rows and state channel c, in the reference's order of precedence
 *          src[c] = -1 - j              -> out[i, j]                                   (the model predicts this channel)
 *          i >= rows - tail, sol[c] >= 0 -> sol[i - (rows - tail), sol[c]]              (insolation, known for any time)
 *          i >= rows - tail, mean        -> mean[c]                                     (impute=True)
 *          i + shift < rows              -> old_state[i + shift, src[c]]                (the data of the later start time)
 *          otherwise                     -> NaN                                         (ran out of data)
 *      old_state / new_state (rows, state_c, hw), out (rows, out_c, hw), sol (tail, sol_planes, hw) | NULL, mean (state_c, hw) |
 *      NULL; float32, planes are copied bit for bit.  new_state must not alias old_state.                                      */
#define DLWP_FB_MAX_CHANNELS 128
typedef struct {
  int rows, state_c, out_c, hw;
  int shift;                        /* k = es + interval - 1: series steps the window advances per model call (0: none)      */
  int tail;                         /* min(es, rows): trailing rows that receive the insolation / the mean state             */
  int sol_planes;                   /* planes per tail row of the insolation block (the input time steps)                    */
  int src[DLWP_FB_MAX_CHANNELS];    /* per state channel: >= 0 channel of the old state; -1 - j: channel j of the output     */
  int sol[DLWP_FB_MAX_CHANNELS];    /* per state channel: plane of the tail row's insolation block, or -1                    */
} dlwp_feedback;
int dlwp_state_feedback(dlwp_handle_t, const void* old_state, const void* out, void* new_state, const void* sol,
                        const void* mean, const dlwp_feedback* fb, int dtype, void* stream);
/* The rollout graph with that update between its calls: call t reads state[t & 1] (state_a = the initial state, written by the
 * caller before every launch; state_b = scratch of the same size), writes its series slot (slot_elems = rows * out_c * hw), and
 * the feedback launch behind it builds state[(t + 1) & 1] with the insolation block sol + t * tail * sol_planes * hw
 * (sol: (calls of the whole rollout - 1, tail, sol_planes, hw) | NULL).  One output per call, one member chain (rows exchange
 * data).  A TIME SLICE of a rollout (one graph per model call, so that a finished slot can leave for the host under the next
 * call): the graph holds calls [first_call, first_call + calls), `series` points at the slot of first_call, feed_last != 0
 * puts the feedback behind its last call into the graph too (every slice but the last); DLWP_ROLLOUT_PREPARED as above.        */
int dlwp_rollout_create_fed(dlwp_handle_t, const dlwp_op* plan, int n_ops, void* const* buffers, int n_buffers,
                            void* state_a, void* state_b, void* series, size_t slot_elems, int calls, int first_call,
                            int feed_last, const dlwp_feedback* fb, const void* sol, const void* mean, int dtype,
                            void* workspace, size_t workspace_bytes, dlwp_rollout_t* out);
/* ---- the returned series of such a forecast (DLWP/model/extensions.py:243-302): one model call's output (n, t, c, hw) -> its
 *      block of the result, time first (kept, n, c, hw) -- the transpose + reshape of :262-263 and the [:, :, :es] cut of :260 --
 *      or (n, kept, c, hw) with keep_time_dim; destination channel j <- source channel perm[j] (NULL: identity): the sorted
 *      (variable, level) order xarray's unstack returns (:298-302).                                                          */
int dlwp_series_arrange(dlwp_handle_t, const void* src, void* dst, int n, int t, int c, int hw, int kept, const int* perm,
                        int time_major, int dtype, void* stream);
int dlwp_rollout_launch(dlwp_rollout_t, void* stream);
int dlwp_rollout_destroy(dlwp_rollout_t);

/* ---- host side of the DataGenerator feed (keras.utils.Sequence batches assembled by worker processes under
 *      fit_generator(use_multiprocessing=True), DLWP/model/models.py:216-228, generators.py:137-159): dst[i] = src[rows[i]],
 *      rows of row_bytes bytes, on `threads` host threads -- straight into the pinned staging buffer of the H2D copy.
 *      Host memory only; no device work, no handle.                                                                          */
int dlwp_host_gather_rows(void* dst, const void* src, const long long* rows, long long n_rows, size_t row_bytes,
                          long long src_rows, int threads);
/* ---- the training step as a library object: replaces the per-step Python launch loop behind keras Model.train_on_batch as
 *      DLWPNeuralNet.fit / fit_generator drive it (DLWP/model/models.py:188-228; examples/train.py:262-263).
 *      A model's step is ~30 launches through this ABI.  Between dlwp_train_step_record_begin and dlwp_train_step_create every
 *      launch-type entry point the RECORDING THREAD calls on the handle is executed as usual and appended to a tape: a closure over
 *      its arguments (descriptors copied; device pointers as given -- the caller keeps that memory alive and in place).  Streams are
 *      recorded as lanes (lane 0 = main_stream), fork / join edges between them go through dlwp_stream_wait.  The step object
 *      replays the tape with ONE C call: DLWP_STEP_LANES issues the launches one by one (lane 0 on the given stream, the others on
 *      the step's own side streams), DLWP_STEP_GRAPH replays one hipGraph captured from that sequence on a single stream (built at
 *      the first launch in that mode), DLWP_STEP_GRAPH_BRANCHES one with the lanes as graph branches.  What varies from step to
 *      step must live in device memory (the Adam step number: dlwp_adam_keras_dev); collectives stay outside.
 *      in_dst / in_floats: the (at most 8) device buffers the recorded launches read the batch and its targets from;
 *      dlwp_train_step_launch(srcs != NULL) copies srcs[i] there first, in one launch.                                        */
#define DLWP_STEP_LANES          0
#define DLWP_STEP_GRAPH          1
#define DLWP_STEP_GRAPH_BRANCHES 2
#define DLWP_STEP_LANES_RECORDED 3  /* as DLWP_STEP_LANES, the side lanes on the streams the step was RECORDED on (the caller keeps them
                                     * alive): streams created later may share a hardware queue with the main stream            */
typedef struct dlwp_train_step* dlwp_train_step_t;
int dlwp_train_step_record_begin(dlwp_handle_t, void* main_stream);
int dlwp_train_step_record_abort(dlwp_handle_t);
int dlwp_stream_wait(dlwp_handle_t, void* waiter_stream, void* signaler_stream);   /* waiter waits for what signaler holds now */
int dlwp_train_step_create(dlwp_handle_t, int n_in, void* const* in_dst, const size_t* in_floats, dlwp_train_step_t* out);
int dlwp_train_step_info(dlwp_train_step_t, int* n_launches, int* n_lanes, int* n_waits);
int dlwp_train_step_launch(dlwp_train_step_t, const void* const* srcs, int mode, void* stream);
int dlwp_train_step_destroy(dlwp_train_step_t);

/* ---- data parallel training: replaces keras.utils.multi_gpu_model (DLWP/model/models.py:104-109, 365-372; batch =
 *      n_gpu x batch, Azure/train_tf.py:163-164).  One process per GPU; every rank holds the whole (< 1 MB) weight set and
 *      trains on its rows of the global batch; the ONE flat fp32 gradient buffer is summed by ONE RCCL all-reduce over
 *      xGMI per step, enqueued on the training stream right behind the last weight-gradient kernel, and dlwp_adam_keras
 *      (grad_scale = 1/world) consumes it on the same stream.  RCCL is bound with dlopen at the first dlwp_comm_* call
 *      (the process' already-loaded librccl.so.1 if there is one), so single-GPU use never touches it.
 *      dlwp_comm_unique_id: id == NULL -> *id_bytes = size needed (128); otherwise rank 0 fills id and the CALLER ships
 *      the bytes to the other ranks (any channel: the launcher's TCP store, MPI, a file).  dlwp_comm_init_rank is
 *      collective over all `world` ranks; `device` is the HIP device of the calling rank.  Buffers are device memory;
 *      both collectives are in place and asynchronous on `stream`.                                                    */
typedef struct dlwp_comm* dlwp_comm_t;
int dlwp_comm_unique_id(void* id, size_t* id_bytes);
int dlwp_comm_init_rank(dlwp_comm_t* comm, int device, int world, int rank, const void* unique_id, size_t id_bytes);
int dlwp_comm_info(dlwp_comm_t, int* world, int* rank, int* rccl_version);
int dlwp_allreduce_sum_f32(dlwp_comm_t, void* flat, size_t n, void* stream);
int dlwp_broadcast_f32(dlwp_comm_t, void* flat, size_t n, int root, void* stream);   /* replicas start identical */
int dlwp_comm_destroy(dlwp_comm_t);

/* ---- a one-shot all-reduce of our own for the same exchange, fused with the Keras-form Adam update (csrc/xchg.hip; SURVEY 5 /
 *      8e: the step's 756 KB buffer is latency-bound -- a ring pays 2 (W - 1) hops, this ONE).  Every rank owns a region of device
 *      memory (header with one flag per rank + two payload buffers, step parity) that its peers map through hipIpcMemHandle (xGMI
 *      peers of one node; on a one-GPU test box two processes of the same device); the region is UNCACHED device memory where the
 *      runtime exports an IPC handle for it (dlwp_xchg_info: memory_kind 2; 1 fine-grained, 0 plain).  One launch per step and
 *      rank, a persistent grid of at most one workgroup per CU whatever n: publish the flat buffer, raise the flag in every peer's
 *      header, wait for the peers' flags (bounded: 2 s; then the launch leaves p / m / v alone, writes NaN over flat[n_params:]
 *      -- the loss table -- and dlwp_xchg_status reports the time-out, for good: the exchange is dead afterwards), read all W
 *      buffers, sum them IN RANK ORDER -- identical bits on every rank -- and update the rank's own parameters.
 *      n (floats, a multiple of 4) is fixed at creation.  RCCL (dlwp_comm_*) stays the default
 *      transport; dlwp_amd/parallel.py takes this one with DLWP_ALLREDUCE=oneshot.
 *      create (every rank) -> exchange the 64-byte handles through any host channel -> connect (world x 64 bytes, rank order).   */
typedef struct dlwp_xchg* dlwp_xchg_t;
int dlwp_xchg_create(dlwp_handle_t, int world, int rank, size_t n_floats, void* ipc_handle_out_64_bytes, dlwp_xchg_t* out);
int dlwp_xchg_connect(dlwp_xchg_t, const void* handles);
int dlwp_xchg_allreduce_sum_f32(dlwp_xchg_t, void* flat, size_t n, void* stream);
int dlwp_xchg_allreduce_adam(dlwp_xchg_t, void* flat, size_t n_params, size_t n, void* p, void* m, void* v, float lr, float beta_1,
                             float beta_2, float epsilon, float decay, long long iteration, float grad_scale, void* stream);
int dlwp_xchg_status(dlwp_xchg_t, int* timed_out);
int dlwp_xchg_info(dlwp_xchg_t, int* memory_kind, int* max_blocks);
int dlwp_xchg_destroy(dlwp_xchg_t);

/* ---- forecast verification on the device (csrc/verify.hip; DLWP/model/verify.py:17-102: forecast_error, persistence_error,
 *      climo_error of the series predict_timeseries(..., return_device=True) leaves in HBM).  dlwp_verify_error_sums reduces the
 *      pairs of two float32 operands described by strides (all in ELEMENTS, all >= 0): at lead f < leads there are
 *      count_f = max(count0 - f * count_dec, 0) pairs of sample rows, row i of operand x starts at
 *      x + f * x_lead_stride + (i + f * x_shift) * x_sample_stride, and a sample row is groups x run contiguous floats.
 *      d = a - b is rounded in float32 (as numpy does on float32 arrays), widened to float64; a NaN d is skipped and not counted
 *      (nanmean; inf - inf included), infinities follow IEEE.  sums (device, (leads, groups, 3) float64) <- sum d^2, sum |d|,
 *      pairs counted; a lead without pairs launches no work and reports three zeros.  With row = groups * run, as
 *      (lead_stride, sample_stride, shift):
 *        forecast_error, valid (F, N, ..):  a = forecast (N*row, row, 0), b = valid (N*row, row, 0), count0 = N,  count_dec = 0
 *        forecast_error, valid (Nv, ..):    a = valid (0, row, 1),        b = forecast (N*row, row, 0), count0 = Nv, count_dec = 1
 *        persistence_error:                 a = valid (0, row, 1),        b = predictors (0, row, 0),   count0 = Nv, count_dec = 1
 *        climo_error:                       a = valid (0, row, 0),        b = mean (0, 0, 0),           count0 = Nv, count_dec = 1
 *      Two launches with a fixed tree (per-thread float64 sums and a 64-bit count; lanes, waves through LDS, one partial per
 *      block in ws; a second kernel sums the partials of each (lead, group) cell), no atomics, no host synchronisation: repeated
 *      calls give identical bits.  16-byte loads when run, all four strides are multiples of 4 and a, b are 16-byte aligned,
 *      scalar loads otherwise (the two routes need not agree in the last float64 bits).  The grid is sized from the handle's
 *      CU count: max(1, 8 * CUs / cells) blocks per cell over the cells of the leads that have pairs, and
 *      dlwp_verify_error_workspace returns leads * groups * B * 24 bytes with B = ceil(8 * CUs / (leads * groups)), enough for
 *      every count0 / count_dec (a NULL handle counts 256 CUs).  Refused without a launch: sizes < 1, negative strides,
 *      null pointers, more than 2^20 cells, a workspace smaller than the launch needs, a null handle (checked in that order).
 *      The caller guarantees that every addressed element exists (dlwp_amd.ops.verify_error_sums checks it).
 *      dlwp_verify_nanmean_samples: x (count, row) contiguous -> mean (row) float32, the NaN-skipping mean over samples,
 *      accumulated in float64 in sample order; a column without a non-NaN sample stores NaN.
 *      Neither is part of a training step: both mark a recording tape foreign.                                             */
size_t dlwp_verify_error_workspace(dlwp_handle_t, int leads, int groups);
int dlwp_verify_error_sums(dlwp_handle_t, const void* a, long long a_lead_stride, long long a_sample_stride, int a_shift,
                           const void* b, long long b_lead_stride, long long b_sample_stride, int b_shift, int leads, int count0,
                           int count_dec, int groups, long long run, void* sums, void* ws, size_t ws_bytes, void* stream);
int dlwp_verify_nanmean_samples(dlwp_handle_t, const void* x, int count, long long row, void* mean, void* stream);

/* ---- month-aware climatology and verification windows (csrc/verify.hip; DLWP/model/verify.py:105-273: monthly_climo_error,
 *      verification_from_samples / _series).  Same conventions as above: float32 data, float64 sums on fixed trees, no atomics,
 *      64-bit offsets, no synchronisation, grids sized from the handle's CU count, all three mark a recording tape foreign.
 *      dlwp_verify_label_nanmean: x (count, row) contiguous float32 -> mean (n_labels, row) float32, the NaN-skipping mean of the
 *      rows that carry each label, n_labels <= 64.  The caller hands the labels over as per-label lists: `offsets` is a HOST array
 *      of n_labels + 1 ints (0 = offsets[0] <= ... <= offsets[n_labels] = count) and `index` a DEVICE array of count ints, the
 *      sample indices of label l at index[offsets[l] .. offsets[l + 1]), ascending.  The list of a label is cut into `split` chunks
 *      [len * k / split, len * (k + 1) / split); a block sums one (label, chunk, 256-thread column tile) in float64 in list order and
 *      stores a (sum, count) pair per column in ws; a second launch adds the chunks in chunk order, divides once and rounds once to
 *      float32 (NaN for a label without a non-NaN sample).  split = min(max(1, 8 * CUs / (n_labels * tiles)), count) with
 *      tiles = ceil(units / 256) and units = row / 4 when row % 4 == 0 and x is 16-byte aligned (16-byte loads), else row: the
 *      sample axis is split only when the column tiles alone do not fill the chip.  dlwp_verify_label_nanmean_workspace returns
 *      n_labels * split * row * 12 bytes for the larger split of the two routes (a NULL handle counts 256 CUs); ws must be 8-byte
 *      aligned.  An index outside [0, count) is skipped, never read.  Refused without a launch: sizes < 1, n_labels outside
 *      1 .. 64, null pointers, offsets that do not run from 0 to count without decreasing, a row too long for one grid, a workspace
 *      that is too small or misaligned, a null handle (in that order).
 *      dlwp_verify_label_error_sums: sums (device, 3 float64) <- sum d^2, sum |d|, pairs counted over d = x[rows[i]] - table[labels[i]],
 *      i < m, with x (count_x, row), table (n_labels, row), rows and labels DEVICE int arrays of m; d is rounded once in float32 and NaN
 *      pairs are skipped, as in dlwp_verify_error_sums, of which this is one cell with the same partial / final tree.  anomaly, if not
 *      NULL, is (m, row) float32 and receives every d, NaN included.  A row index or label outside its range gives a NaN row and is
 *      never used as an address.  16-byte accesses when row % 4 == 0 and x, table and anomaly are 16-byte aligned.  ws: what
 *      dlwp_verify_error_workspace(h, 1, 1) returns.
 *      dlwp_gather_rows_fill: src (src_rows, row) float32, rows a DEVICE array of n int64 -> dst (n, row): dst[j] = src[rows[j]]
 *      with the bits copied (NaN payloads included), or quiet NaNs (0x7fc00000) across the row where rows[j] < 0 -- reindex without a
 *      fill method.  An index >= src_rows is the caller's error (dlwp_amd.ops.gather_rows_fill refuses it on the host array); the
 *      kernel stores NaN for it and reads nothing.  16-byte accesses when row % 4 == 0 and src, dst are 16-byte aligned; n == 0 is a
 *      no-op.                                                                                                                      */
size_t dlwp_verify_label_nanmean_workspace(dlwp_handle_t, int count, long long row, int n_labels);
int dlwp_verify_label_nanmean(dlwp_handle_t, const void* x, int count, long long row, const int* offsets, const void* index,
                              int n_labels, void* mean, void* ws, size_t ws_bytes, void* stream);
int dlwp_verify_label_error_sums(dlwp_handle_t, const void* x, int count_x, long long row, const void* rows, const void* labels, int m,
                                 const void* table, int n_labels, void* anomaly, void* sums, void* ws, size_t ws_bytes, void* stream);
int dlwp_gather_rows_fill(dlwp_handle_t, const void* src, long long src_rows, long long row, const void* rows, long long n, void* dst,
                          void* stream);

/* ---- climatological quantiles (csrc/quantile.hip; no counterpart in the reference module: the per-point event thresholds of
 *      dlwp_ens_event_counts -- terciles, "the 95th percentile of this month" -- from the record itself).  Conventions as above:
 *      float32 data, 64-bit offsets, no synchronisation, no atomics; the selection counts integers, so the result does not depend on
 *      scheduling and there is no float64 sum.  dlwp_verify_label_quantiles marks a recording tape foreign.
 *      dlwp_verify_label_quantiles: x (count, row) contiguous float32, labels as the per-label lists of dlwp_verify_label_nanmean
 *      (`offsets` HOST, n_labels + 1 ints; `index` DEVICE, count ints; an index outside [0, count) is skipped, never read), q a HOST
 *      array of k probabilities, 1 <= k <= 8, each finite and in [0, 1] -> out (k, n_labels, row) float32 and, if counts is not NULL,
 *      counts (n_labels, row) int32, the non-NaN samples.  Per (label, column): NaNs (v != v) are dropped, n values are left; every
 *      output of the column is the quiet NaN 0x7fc00000 when n == 0.  The values are ordered by the unsigned key of their bits u
 *      (u ^ 0xffffffff with the sign bit set, else u | 0x80000000: a total order, -0.0 < +0.0, infinities at the ends) into
 *      s[0] <= ... <= s[n - 1]; h = (n - 1) * q is ONE float64 product, and
 *        DLWP_QUANTILE_LOWER    s[floor(h)]           DLWP_QUANTILE_HIGHER   s[ceil(h)]
 *        DLWP_QUANTILE_NEAREST  s[rint(h)], halves to even
 *        DLWP_QUANTILE_LINEAR   a = s[floor(h)], b = s[min(floor(h) + 1, n - 1)], g = h - floor(h): a when g == 0, else
 *                               float32(a + (b - a) * g), every operation rounded once in float64 (no fused multiply-add) and the
 *                               sum rounded once to float32; a NaN result (inf - inf) is stored as 0x7fc00000.
 *      The order statistics keep the bits of the sample (the sign of a zero included).  numpy.nanquantile on a float64 copy, rounded to
 *      float32, gives the same values.  Algorithm: bisection on the key, most significant bit first -- 32 sweeps over the column's
 *      keys, each counting for every rank the keys below prefix | bit -- after one sweep that counts n.
 *      route 1, LDS: a workgroup of four waves owns (label, tile of cols adjacent columns), gathers the label's rows of the tile into
 *      LDS once as keys (16-byte loads when row % 4 == 0 and x is 16-byte aligned, else scalar) and sweeps there; cols is the widest
 *      of 64, 32, 16 with round_up(max_len, 256 / cols) * cols * 4 <= 81920 bytes (half of the CU's 160 KiB: two workgroups per CU),
 *      max_len the longest list: 320, 640 or 1280 rows.  route 2, streaming: the same sweeps read x through the index list (33 reads
 *      of the label's rows, 64 columns per workgroup); no limit on max_len.  route 0: LDS when max_len fits, else streaming.  Both
 *      routes return the same bits.  dlwp_verify_label_quantiles_plan reports the choice (route_out: 1 or 2) and the tile width
 *      (cols_out) for a longest list of max_len rows; it needs no handle.  dlwp_verify_label_quantiles_workspace returns
 *      n_labels * row * 4 bytes rounded up to 16 (0 for sizes it refuses): ws receives the counts when `counts` is NULL, and must be
 *      16-byte aligned.
 *      Refused without a launch, in this order: count or row < 1, n_labels outside 1 .. 64, k outside 1 .. 8, a q that is NULL, not
 *      finite or outside [0, 1], an unknown method, an unknown route, null pointers (x, offsets, index, out, ws), offsets that do not
 *      run from 0 to count without decreasing, a row too long for one grid, route 1 with a list that does not fit, a workspace that is
 *      too small or misaligned, a null handle.                                                                                     */
#define DLWP_QUANTILE_LINEAR  0
#define DLWP_QUANTILE_LOWER   1
#define DLWP_QUANTILE_HIGHER  2
#define DLWP_QUANTILE_NEAREST 3
int dlwp_verify_label_quantiles_plan(dlwp_handle_t, int max_len, long long row, int route, int* route_out, int* cols_out);
size_t dlwp_verify_label_quantiles_workspace(dlwp_handle_t, int count, long long row, int n_labels, int k);
int dlwp_verify_label_quantiles(dlwp_handle_t, const void* x, int count, long long row, const int* offsets, const void* index,
                                int n_labels, const double* q, int k, int method, int route, void* out, void* counts /* may be NULL */,
                                void* ws, size_t ws_bytes, void* stream);

/* ---- latitude-weighted forecast skill (csrc/skill.hip; no counterpart in the reference module, which stops at unweighted mse / mae /
 *      rmse; the anomaly correlation is the reference's training metric, DLWP/custom.py anomaly_correlation).  dlwp_verify_skill_sums
 *      reads a forecast fc and an observation ob addressed exactly as a and b of dlwp_verify_error_sums (strides in ELEMENTS, all
 *      >= 0; lead f has count_f = max(count0 - f * count_dec, 0) pairs of sample rows; row i of operand x starts at
 *      x + f * x_lead_stride + (i + f * x_shift) * x_sample_stride; a sample row is groups x run contiguous floats) and adds
 *        a climatology: climo (n_labels, groups * run) float32, n_labels in 1 .. 64, NULL = zero; labels a DEVICE int32 array, the
 *          label of pair (f, i) is labels[f * label_lead_stride + i + f * label_shift], NULL = label 0.  A label outside
 *          [0, n_labels) skips the pair and is never used as an address.  c = climo[label][position of the pair in its row];
 *        weights: w_len DEVICE floats, NULL = all ones; element e of a group's run has weight weights[(e / w_inner) % w_len], and
 *          run % (w_inner * w_len) == 0.  For an (..., H, W) row: w_len = H, w_inner = W.
 *      Per pair d = fc - ob, fa = fc - c, oa = ob - c are each rounded once in float32 (fa, oa are the inputs themselves without a
 *      table); a pair with a NaN among d, fa, oa is skipped in every sum and in the count, infinities follow IEEE; everything behind
 *      that is float64.  sums (device, (leads, groups, 10) float64) <-
 *        0: sum w      1: sum w d     2: sum w d^2    3: sum w |d|    4: sum w fa
 *        5: sum w oa   6: sum w fa oa 7: sum w fa^2   8: sum w oa^2   9: pairs counted
 *      and a lead without pairs launches no work and reports ten zeros.  The tree is dlwp_verify_error_sums': per-thread float64
 *      sums and a 64-bit count, lanes, waves through LDS, one partial (ten doubles) per block in ws, a second kernel that adds the
 *      partials of a cell in index order; no atomics, no host synchronisation, identical bits on repeated calls; max(1, 8 * CUs /
 *      cells) blocks per cell over the cells of the leads that have pairs.  16-byte loads when run and the four operand strides are
 *      multiples of 4 and fc, ob, climo are 16-byte aligned, scalar loads otherwise; with 16-byte loads the weight is looked up once
 *      per unit when w_inner % 4 == 0 and per element otherwise (a unit may then straddle two latitude rows).
 *      dlwp_verify_skill_workspace returns leads * groups * B * 80 bytes, B = ceil(8 * CUs / (leads * groups)) (a NULL handle counts
 *      256 CUs); ws must be 8-byte aligned.  Refused without a launch, in this order: sizes < 1; negative strides, shifts or
 *      count_dec; n_labels outside 1 .. 64 with a table; labels without a table; w_len < 1, w_inner < 1 or a run they do not
 *      divide, with weights; null fc, ob or sums; more than 2^20 cells; a workspace too small or misaligned; a null handle.
 *      The caller guarantees that every addressed element exists (dlwp_amd.ops.verify_skill_sums checks it).  Marks a recording
 *      tape foreign.                                                                                                        */
size_t dlwp_verify_skill_workspace(dlwp_handle_t, int leads, int groups);
int dlwp_verify_skill_sums(dlwp_handle_t, const void* fc, long long fc_lead_stride, long long fc_sample_stride, int fc_shift,
                           const void* ob, long long ob_lead_stride, long long ob_sample_stride, int ob_shift, int leads, int count0,
                           int count_dec, int groups, long long run, const void* climo, int n_labels, const void* labels,
                           long long label_lead_stride, int label_shift, const void* weights, int w_len, long long w_inner,
                           void* sums, void* ws, size_t ws_bytes, void* stream);

/* ---- forecast skill per grid point (csrc/skill_map.hip): the sums of dlwp_verify_skill_sums reduced over the SAMPLES of a lead at
 *      every point of the sample row, and the scores made from them on the device.  fc, ob, climo and labels are addressed exactly as
 *      in dlwp_verify_skill_sums with groups = 1 and run = row; there are no weights (a weight is constant per point and cancels).
 *      Per pair d = fc - ob, fa = fc - c, oa = ob - c are each rounded once in float32; a pair with a NaN among them, or with a label
 *      outside [0, n_labels), is skipped for that point only and is never used as an address; everything behind that is float64.
 *        sums   (leads, 9, row) float64 planes   0: sum d    1: sum d^2   2: sum |d|   3: sum fa   4: sum oa   5: sum fa oa
 *                                                6: sum fa^2 7: sum oa^2  8: pairs counted
 *        scores (leads, 6, row) float32 planes   mse, rmse, mae, bias, acc, acc_centered: the formulas of dlwp_amd.model.verify.
 *                                                finish_skill with S0 = the count, each operation rounded once in float64 (nothing
 *                                                is contracted into a fused multiply-add), cast once; NaN where nothing was counted
 *                                                or a denominator is not positive
 *        counts (leads, row) int32
 *      Each of the three may be NULL, not all of them.  A lead without pairs stores zero sums, NaN scores and zero counts.
 *      A thread owns one unit of one lead -- four adjacent points with 16-byte loads when row and the four operand strides are
 *      multiples of 4 and fc, ob, climo are 16-byte aligned, else one point (the two routes give the same bits) -- and adds that lead's
 *      samples in sample order, several in flight; the label is the same in every lane.  The sample axis is cut into `split` chunks
 *      [cnt_f k / split, cnt_f (k + 1) / split): split = 0 asks for min(max(1, 8 CUs / (leads * tiles)), count0) with tiles =
 *      ceil(units / 256), i.e. the samples are split only when leads x column tiles do not fill the chip; a positive split is taken as
 *      given; either is capped at count0 and is at least 1.  With one chunk the launch finishes by itself; with more, the chunks'
 *      planes go to ws and a second launch adds them in chunk order and finishes.  No atomics, no host synchronisation, identical
 *      bits on repeated calls (a different split is a different order of additions).  dlwp_verify_skill_map_workspace returns
 *      leads * split * 9 * row * 8 bytes for the split the call will use (0 for one chunk; for split = 0 that of the 16-byte route,
 *      the larger one; a NULL handle counts 256 CUs); ws must be 8-byte aligned.  Refused without a launch, in this order: leads or
 *      row < 1; negative strides, shifts or count_dec; n_labels outside 1 .. 64 with a table; labels without a table; null fc or
 *      ob, or all three outputs NULL; split < 0; a row too long for one grid (leads * split * tiles >= 2^31); a workspace too small or
 *      misaligned; a null handle.  The caller guarantees that every addressed element exists (dlwp_amd.ops.verify_skill_map checks).
 *      dlwp_verify_skill_map_finish does the last step alone, for tables that were added over ranks or sample chunks: sums is ONE
 *      table of 9 planes of `cells` float64 (one lead of the layout above, cells = row), scores 6 planes of `cells` float32, counts
 *      `cells` int32, either of the two may be NULL.  Refused in this order: cells < 1; null sums or no output; too many cells for one
 *      grid; a null handle.  Both mark a recording tape foreign.                                                                    */
size_t dlwp_verify_skill_map_workspace(dlwp_handle_t, int leads, int count0, long long row, int split);
int dlwp_verify_skill_map(dlwp_handle_t, const void* fc, long long fc_lead_stride, long long fc_sample_stride, int fc_shift,
                          const void* ob, long long ob_lead_stride, long long ob_sample_stride, int ob_shift, int leads, int count0,
                          int count_dec, long long row, const void* climo, int n_labels, const void* labels,
                          long long label_lead_stride, int label_shift, int split, void* sums, void* scores, void* counts, void* ws,
                          size_t ws_bytes, void* stream);
int dlwp_verify_skill_map_finish(dlwp_handle_t, const void* sums, long long cells, void* scores, void* counts, void* stream);

/* ---- zonal power spectra of a forecast and its verification (csrc/spectrum.hip; no counterpart in the reference module).  fc and ob
 *      are addressed exactly as in dlwp_verify_skill_sums (strides in ELEMENTS, all >= 0; lead f has count_f = max(count0 - f *
 *      count_dec, 0) pairs of sample rows; row i of operand x starts at x + f * x_lead_stride + (i + f * x_shift) * x_sample_stride; a
 *      sample row is groups x run contiguous floats).  A group's run is run / width LONGITUDE ROWS of `width` floats (4 <= width <=
 *      512, run % width == 0); longitude row r of a run has weight weights[r % w_len] (w_len DEVICE floats, (run / width) % w_len ==
 *      0; NULL = all ones).  twiddles: 2 * width DEVICE floats, cos(2 pi m / width) for m < width, then sin(2 pi m / width), computed
 *      in float64 and rounded once (dlwp_amd.ops.spectrum_twiddles).
 *      Per longitude row, d = fc - ob is rounded once in float32; O = rfft(ob), D = rfft(d) at the K = width / 2 + 1 wavenumbers (the
 *      forecast's transform is O + D).  A row with a non-finite value among fc, ob, d is skipped whole, in every sum and in the count.
 *      With c_0 = 1, c_k = 2, c_{width/2} = 1 for an even width, all over width^2 (sum_k c_k |X_k|^2 is the mean of x^2 of a row):
 *        sums (device, (leads, groups, 4, K) float64) <-  0: sum w c_k |O_k|^2          1: sum w c_k |D_k|^2
 *                                                          2: sum w c_k Re(D_k conj O_k) 3: sum w c_k Im(D_k conj O_k)
 *        norm (device, (leads, groups, 2) float64)    <-  sum w, longitude rows counted
 *      over the longitude rows of all pairs of the lead; a lead without pairs launches no work and reports zeros.
 *      The transform is a product on v_mfma_f32_32x32x2_f32 (exact float32, a j-ordered fmaf chain): the row's mean m = fl32(float64
 *      row sum / width) is taken out first, y_j = fl32(x_j - m), and X_0 is the float64 row sum itself; the row is folded, e_j = y_j +
 *      y_{width-j} against the cosines and o_j = y_j - y_{width-j} against the sines, j <= width / 2, so a coefficient is a chain of
 *      K products (padded with zeros to an even number); the twiddle of (j, k) is entry (j k) mod width of the table, gathered from
 *      LDS.  Behind the product everything is float64: re and im widened, the four terms weighted and added over the rows of a
 *      32-row tile in registers, per thread over the tiles of a block, one partial (4 K + 2 doubles) per block in ws, a second launch
 *      that adds the partials of a cell in index order.  No atomics, no host synchronisation, identical bits on repeated calls;
 *      max(1, 8 * CUs / cells) blocks per cell over the cells of the leads that have pairs, at most one per 32-row tile of lead 0.
 *      16-byte loads when width and the four operand strides are multiples of 4 and fc, ob are 16-byte aligned, scalar loads
 *      otherwise (the same bits).  dlwp_verify_spectrum_workspace returns leads * groups * B * (4 K + 2) * 8 bytes, B = ceil(8 * CUs /
 *      (leads * groups)) (a NULL handle counts 256 CUs; 0 for sizes it refuses); ws must be 8-byte aligned.  Refused without a
 *      launch, in this order: leads, groups or run < 1; negative strides, shifts or count_dec; width outside 4 .. 512 or not dividing
 *      run; w_len < 1 or not dividing run / width, with weights; null fc, ob, twiddles, sums or norm; more than 2^20 cells, or 2^31
 *      longitude rows in a cell; a workspace too small or misaligned; a null handle.  The caller guarantees that every addressed
 *      element exists (dlwp_amd.ops.verify_spectrum_sums checks it).  Marks a recording tape foreign.                        */
size_t dlwp_verify_spectrum_workspace(dlwp_handle_t, int leads, int groups, int width);
int dlwp_verify_spectrum_sums(dlwp_handle_t, const void* fc, long long fc_lead_stride, long long fc_sample_stride, int fc_shift,
                              const void* ob, long long ob_lead_stride, long long ob_sample_stride, int ob_shift, int leads, int count0,
                              int count_dec, int groups, long long run, int width, const void* weights, int w_len,
                              const void* twiddles, void* sums, void* norm, void* ws, size_t ws_bytes, void* stream);

/* ---- batches of a series generator cut out of an HBM-resident series (csrc/series.hip; DLWP/model/generators.py:323-629,
 *      SeriesDataGenerator.generate).  One launch fills X and every target block of a batch:
 *        dst[g.dst][i * row_d + g.dst_at + e] = src[g.src][(samples[i] + g.shift) * row_s + g.src_at + e],  e < g.len, i < n
 *      for every segment g of the table.  srcs[s] = {base, rows, row}: a DEVICE float32 array (rows, row), one row per time (the
 *      input series, the output series, the insolation series), at most 4.  dsts[d] = {base, row}: a DEVICE float32 array (n, row)
 *      (X and each target block), at most 32.  segs: a HOST array of at most 64 segments, in floats; it is validated here and handed
 *      to the kernel by value with the two descriptor tables (3.4 of the 4 KiB of kernel arguments).  samples: a DEVICE array of n
 *      int64 start positions.  A segment is a run that is contiguous on both sides; src_at lies inside the source row and the run
 *      may continue over the row's end into the following times (the consecutive states of a window are one run).  The bits are
 *      copied as words, NaN payloads included.  A run whose first time samples[i] + shift or whose last time is no row of the source
 *      is stored as quiet NaNs (0x7fc00000) over its whole length and is never used as an address.  16-byte accesses when every
 *      row, src_at, dst_at and len is a multiple of 4 floats and every base is 16-byte aligned, one float at a time otherwise
 *      (decided on the host).  A 256-thread block moves a chunk of 1024 units of one segment of one sample per turn (a unit = 16
 *      bytes or one float; four loads in front of four stores per thread); the grid is min(n * chunks per sample,
 *      dlwp_series_gather_grid_cap(h) = 8 * CUs) blocks, which stride over the (sample, chunk) list.  No atomics, no LDS, no
 *      synchronisation; not part of a training step: it marks a recording tape foreign.  Refused without a launch, in this order:
 *      n_src, n_dst, n_seg outside 1 .. 4 / 32 / 64 or n < 0; a null table; per source a null base, rows or row < 1, a size that
 *      overflows; per destination a null base, row < 1, n * row overflowing; per segment a source or destination index outside
 *      its table, len < 1, src_at outside [0, row_s), dst_at + len past row_d, a len or shift that overflows.  n == 0 is then a
 *      no-op; otherwise a null `samples` and a null handle are refused.  The caller guarantees that the arrays hold what the
 *      descriptors say (dlwp_amd.ops.series_window_gather checks it).                                                              */
#define DLWP_SERIES_MAX_SRCS 4
#define DLWP_SERIES_MAX_DSTS 32
#define DLWP_SERIES_MAX_SEGS 64
typedef struct dlwp_series_src { const void* base; long long rows, row; } dlwp_series_src;
typedef struct dlwp_series_dst { void* base; long long row; } dlwp_series_dst;
typedef struct dlwp_series_seg { int src, dst; long long shift, src_at, dst_at, len; } dlwp_series_seg;
int dlwp_series_gather_grid_cap(dlwp_handle_t);
int dlwp_series_window_gather(dlwp_handle_t, const dlwp_series_src* srcs, int n_src, const dlwp_series_dst* dsts, int n_dst,
                              const dlwp_series_seg* segs, int n_seg, const void* samples, long long n, void* stream);

/* ---- ensemble verification on the device (csrc/ensemble.hip; the reference averages members on the host,
 *      examples/plot_ensemble.py:242,269): reductions ACROSS the member axis of the series predict_timeseries(...,
 *      return_device=True) leaves in HBM.  A column is one (lead t, sample s, point p) with `members` float32 values
 *        x[t * lead_stride + s * sample_stride + i * member_stride + p],  i < members, p < row,
 *      all strides in ELEMENTS and >= 0; consecutive points are contiguous.  The two layouts of a contiguous series of row floats:
 *
 *        series viewed as        lead_stride   sample_stride   member_stride
 *        (T, S, M, row)          S * M * row   M * row         row
 *        (T, M, S, row)          M * S * row   row             S * row
 *
 *      All per-column arithmetic is float64 on the float32 values: mean = (sum_i x_i) / M in member order; with d_i = x_i - x_0
 *      (exact), var_ddof = (sum d_i^2 - (sum d_i)^2 / M) / (M - ddof) and spread = sqrt(max(var, 0)).
 *      dlwp_ens_mean_spread: mean, spread (leads, samples, row) float32, either may be NULL (not both); NaN where a member is NaN.
 *      One pass over the members, a thread owns four adjacent columns (16-byte accesses: row and the three strides multiples of 4,
 *      all bases 16-byte aligned) or one.  2 <= members, ddof 0 or 1.
 *      dlwp_ens_score_sums: y is the contiguous verification (leads, samples, groups * run) float32 and row = groups * run.  Per
 *      (lead, group) cell, over the columns where neither y nor a member is NaN:
 *        sums[cell][0..5] = sum (mean - y)^2, sum |mean - y|, sum var_0, sum A, sum B, columns counted      (float64)
 *        hist[cell][r]    = columns with r = #{i : x_i < y}, r = 0 .. members (ties count as not below)       (int64)
 *      with A = (1/M) sum_i |x_i - y| and B = sum_{i<j} |x_i - x_j| = sum_k (2k - M + 1) x_(k) over the ascending order, so that
 *      crps = A - B / M^2 and fair_crps = A - B / (M (M - 1)).  crps_out, if not NULL, is (leads, samples, groups * run) float32 and
 *      receives every column's crps, NaN for a skipped column.  2 <= members <= 256, any integer.  A wave owns 64 adjacent points;
 *      a lane keeps 32 members of its column in registers, sorts them with an unrolled bitonic network on order-preserving integer
 *      keys and, above 32 members, parks the sorted runs in LDS ([member][point], a lane only ever touches its own column: no bank
 *      conflicts, no barriers) and merges up to 8 runs head by head while it accumulates B.  Sums are two-stage on a fixed tree
 *      (lanes, one partial per block in ws, a second launch adds a cell's partials in index order); the histogram uses integer LDS
 *      atomics inside a block and the same second launch: no global atomics, repeated calls give identical bits.
 *      dlwp_ens_score_workspace returns the bytes of ws for any sample count (a NULL handle counts 256 CUs), 0 for sizes outside the
 *      ranges above.  ws must be 8-byte aligned.  Refused without a launch: sizes out of range, negative strides, null pointers, more
 *      than 2^20 cells, a workspace too small or misaligned, a null handle (in that order).  The caller guarantees that every
 *      addressed element exists (dlwp_amd.ops checks it).  None is part of a training step: all mark a recording tape foreign.   */
int dlwp_ens_mean_spread(dlwp_handle_t, const void* x, int leads, int samples, int members, long long lead_stride,
                         long long sample_stride, long long member_stride, long long row, int ddof, void* mean, void* spread,
                         void* stream);
size_t dlwp_ens_score_workspace(dlwp_handle_t, int leads, int groups, int members);
int dlwp_ens_score_sums(dlwp_handle_t, const void* x, long long lead_stride, long long sample_stride, long long member_stride,
                        const void* y, int leads, int samples, int members, int groups, long long run, void* sums, void* hist,
                        void* crps_out, void* ws, size_t ws_bytes, void* stream);

/* ---- ensemble EVENT verification on the device (csrc/events.hip): columns, strides, layouts and groups are
 *      those of the block above, row = groups * run.  thr holds `thresholds` (K, 1 .. 8) float32 thresholds per group,
 *      (K, groups), with thr_per_point == 0 -- uniform within a group, loaded once per block -- or per point, (K, groups * run), with
 *      thr_per_point == 1.  With below == 0 member i shows the event where x_i > thr and the event verified where y > thr; with
 *      below == 1 the tests are x_i < thr and y < thr.  Comparisons are made on the float32 values; ties are no event.
 *        n = #{i : event_i} in 0 .. members,  o = 1 if the event verified, else 0
 *        table[lead][group][k][n][o] = columns of the cell with that n and o, over the columns where y is not NaN, no member
 *                                      is NaN and thr is not NaN                                                     (int64)
 *        prob_out[k][lead][sample][p] = float32(double(n) / double(members)); NaN where a member or thr is NaN; y plays no part
 *      table is (leads, groups, K, members + 1, 2); prob_out is (K, leads, samples, groups * run) float32; y is the contiguous
 *      verification (leads, samples, groups * run).  y and table are both given or both NULL, at least one of table / prob_out
 *      is given, and ws is needed only with table.  2 <= members <= 256.  One pass over the members with K counters per column in
 *      registers; a lane owns four adjacent columns (16-byte accesses: run and the three strides multiples of 4, x, y, prob_out
 *      and a per-point thr 16-byte aligned) or one.  A block keeps its table in LDS as up to 32 interleaved replicas (a lane
 *      adds to replica lane mod replicas, so a wave's adds spread over the banks whatever the data are); where the table leaves
 *      room for fewer than 16, a wave first aggregates equal bins (first remaining lane's bin, ballot, one add of the population
 *      count; at most 4 rounds) and the lanes still left use plain LDS adds.  Each block writes its 32-bit partial table to ws
 *      and a second launch adds a cell's partials in index order: no global atomics, repeated calls give identical bits.
 *      dlwp_ens_event_workspace returns the bytes of ws for any sample count (a NULL handle counts 256 CUs), 0 for sizes outside
 *      the ranges.  ws must be 4-byte aligned.  Refused without a launch, in this order: sizes or flags out of range (leads,
 *      samples, groups, run >= 1; members 2 .. 256; thresholds 1 .. 8; both flags 0 or 1), negative strides, the null-pointer rules
 *      above, more than 2^20 cells (or more columns per block than a 32-bit partial counts), a workspace too small or
 *      misaligned, a null handle.  The caller guarantees that every addressed element exists (dlwp_amd.ops checks it).  Not
 *      part of a training step: it marks a recording tape foreign.                                                            */
size_t dlwp_ens_event_workspace(dlwp_handle_t, int leads, int groups, int members, int thresholds);
int dlwp_ens_event_counts(dlwp_handle_t, const void* x, long long lead_stride, long long sample_stride, long long member_stride,
                          const void* y, const void* thr, int thr_per_point, int below,
                          int leads, int samples, int members, int groups, long long run, int thresholds,
                          void* table, void* prob_out, void* ws, size_t ws_bytes, void* stream);

/* ---- the ensemble member generator (csrc/perturb.hip; the reference has no counterpart): a perturbed-
 *      initial-condition ensemble made in HBM.  x: float32 (samples, channels, height, width) contiguous; sigma: float32[channels];
 *        out[s * sample_stride + m * member_stride + (k * height + i) * width + j] = x[s, k, i, j] + sign * sigma[k] * zeta
 *      for m < members, strides in ELEMENTS (the two layouts of the table above: (S, M, row) has sample_stride = M * row and
 *      member_stride = row; (M, S, row) has sample_stride = row and member_stride = S * row), the product and the sum each rounded
 *      once to float32.  Global member g = first_member + m; with `control`, member g == 0 is x itself bit for bit and p = g - 1,
 *      otherwise p = g; with `antithetic`, draw d = p >> 1 and sign = -1 for odd p, otherwise d = p and sign = +1.
 *      White noise z(d, s, k, i, j), defined for every VIRTUAL row |i| < 32768: Philox-4x32-10 with key (seed low, seed high) and
 *      counter (j >> 2, (i + 32768) + 65536 k, d, s); words (w0, w1) give columns 4q, 4q + 1 and (w2, w3) columns 4q + 2, 4q + 3 by
 *        u1 = (2 (wa >> 9) + 1) 2^-24, u2 = (wb >> 8) 2^-24, r = sqrt(-2 ln u1), z_even = r cos(2 pi u2), z_odd = r sin(2 pi u2).
 *      zeta(i, j) = sum_a taps_y[a + radius_y] sum_b taps_x[b + radius_x] z(i + a, (j + b) mod width): the longitude pass first, then
 *      latitude, taps in ascending order, float32 accumulators from 0 (the caller normalises the taps to sum g^2 = 1; radius 0 with
 *      tap 1 is white noise).  Both radii 0: no LDS, a lane owns a column quad and stores it for every member it is given (16-byte
 *      accesses where width and both strides are multiples of 4 and x, out are 16-byte aligned).  Otherwise a workgroup stages a
 *      32 x 64 tile of white noise plus its halo in LDS; the wrap and the rows beyond the grid come from the counter, not from memory.
 *      No atomics, no workspace, no synchronisation; the same bits on every run, for every split of the members over calls and
 *      in both layouts.  NaN in x stays NaN at that element only.  Refused without a launch, in this order: sizes < 1, members < 1,
 *      first_member < 0, a radius outside 0 .. 16, radius_x > width, channels >= 65536, height + radius_y >= 32768, flags other
 *      than 0 / 1, sizes too large for one grid, output strides that overlap, null or misaligned pointers, a null handle.
 *      Not part of a training step: it marks a recording tape foreign.                                                      */
#define DLWP_ENS_MAX_RADIUS 16
typedef struct {
  int samples, channels, height, width;
  int members, first_member;
  unsigned long long seed;
  int radius_y, radius_x;
  float taps_y[2 * DLWP_ENS_MAX_RADIUS + 1], taps_x[2 * DLWP_ENS_MAX_RADIUS + 1];   /* taps_*[a + radius], a = -radius .. radius */
  int control, antithetic;
  long long sample_stride, member_stride;
} dlwp_ens_perturb_desc;
int dlwp_ens_perturb(dlwp_handle_t, const void* x, const void* sigma, void* out, dlwp_ens_perturb_desc d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DLWP_HIP_H */
