/*
 * helmnet_hip.h -- C ABI of libhelmnet_hip.so, the MI355X (gfx950) implementation of the
 * helmnet IterativeSolver inference hot path.
 *
 * The reference (ucl-bug/helmnet) is pure Python/PyTorch and defines NO plugin / operator /
 * FFI interface: its boundary is the Python surface of
 * `IterativeSolver`.  This header is the C boundary introduced underneath that surface; each
 * entry point names the reference code it replaces (paths relative to the reference root).
 * The Python class `helmnet_amd.IterativeSolver` binds these symbols with ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - every function returns 0 on success and a negative hn_status on failure; the message
 *     is available from hn_last_error(ctx) (or hn_last_error(NULL) for hn_create failures).
 *     No exception crosses the ABI, no global mutable state except that last-error string; environment
 *     variables are read once per context, in hn_create, as defaults for hn_set_unet_precision / hn_set_option.
 *   - every entry point selects the context's device for its own duration and restores the caller's.
 *   - all tensor arguments are DEVICE pointers to contiguous fp32, NCHW, owned by the caller,
 *     who guarantees their lifetime until `stream` has been synchronised.
 *   - alignment and overlap.  ALIGNMENT: a tensor argument needs the alignment of its element type and no more -- 4 bytes for fp32 and int32, 8 for
 *     the doubles of the _f64 family, 1 for hn_adam_step's mask -- so a view carved out of a larger allocation (a replay buffer, a history, a flat
 *     workspace) is a valid argument.  This holds for hn_laplacian, hn_residual, hn_residual_vjp, hn_rmse, hn_unet, hn_step, hn_double_conv, hn_conv8x8,
 *     hn_out_conv, hn_get_sigmas, hn_laplacian_f64, hn_residual_f64, hn_unet_f64, hn_step_f64, hn_train_grad, hn_step_vjp, hn_step_jvp, hn_adam_step, hn_train_peek,
 *     hn_stream_verdict and hn_rows_gather / hn_rows_scatter (which copy with 16-byte accesses where pointers and rows allow it and element by element
 *     otherwise).  The exceptions name their requirement and refuse otherwise with HN_ERR_ARG: 16 bytes for the fields of hn_gmres_cycle, hn_fgmres_cycle
 *     and their _refine_ forms, and for hn_stream_swap.  Alignment can cost speed, never results beyond fp32 rounding: where wf, res or the hidden states
 *     of hn_step / hn_unet are not 16-byte aligned, the kernels that stage them with 16-byte LDS-direct loads stand down -- the level-0 DoubleConvs
 *     (HN_OPT_DC_VALU 3 / 4, and with them the paired launch of HN_OPT_DC_PAIR) run on hn_dcv.hip, which agrees to fp32 rounding (4e-6 * max), and the
 *     hidden-state DoubleConvs (HN_OPT_STATE_KERNEL) on the general kernel, bit-identical; every other kernel, the spectral operator included, is the
 *     same for every alignment and gives the same bits.
 *     OVERLAP: no tensor a call WRITES may overlap any other tensor of that call; tensors that are only read may share memory.  Checked, with
 *     HN_ERR_ARG naming the two arguments and nothing enqueued, by hn_step (one tolerated form, see there), hn_unet, hn_step_jvp, the _f64 family and the GMRES
 *     family; hn_residual_vjp refuses g == out.  The other entry points (hn_laplacian, hn_residual, hn_rmse, the three sub-module calls, hn_train_grad,
 *     hn_step_vjp, hn_adam_step, hn_rows_*, hn_stream_swap beyond its own slot rules) do not check: an output that overlaps an input or another
 *     output there gives undefined values (never an access outside the caller's tensors).
 *   - all work is enqueued asynchronously on the caller's `stream` (a hipStream_t passed as
 *     void*; NULL = the default stream).  A ctx is bound to one device and is NOT thread-safe.
 *     ONE exception, "side streams": hn_step and hn_train_grad run part of their work on library streams beside the caller's, and HIP
 *     deals streams onto a few hardware queues -- a library stream that shares the caller's queue silently serialises (inference -9 %,
 *     the training step up to 3 x).  So the FIRST call that meets a new caller stream (per context and entry point) PROBES the library's
 *     candidate streams against it: it synchronises that stream (hipStreamSynchronize), runs a 200 us spin kernel on it and an empty
 *     kernel on a candidate, up to three times per candidate (majority), ~1 ms in all, and remembers the answer for that stream -- later
 *     calls on any already-probed stream are asynchronous again.  The probe never runs while the caller's stream (or a stream it is
 *     compared with) is being captured; a first call under capture uses candidate 0 unprobed.  A capture in global mode on ANOTHER thread
 *     cannot be detected: make the first call before it, or disable probing.  HN_SIDE_PRIORITY=1 / 2 / 3 in the environment (lowest /
 *     normal / highest priority candidate) disables probing altogether.  hn_get_counter(HN_CNT_STREAM_PROBES) counts the probes.
 *   - the library owns only its ctx: a re-packed copy of the weights, the spectral tables
 *     and the activation workspace (grown on demand by hn_reserve / the first call).
 */
#ifndef HELMNET_HIP_H
#define HELMNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hn_ctx hn_ctx;

enum hn_status {
    HN_OK = 0,
    HN_ERR_ARG = -1,      /* bad argument (shape, NULL pointer, unsupported size)            */
    HN_ERR_STATE = -2,    /* call order: weights / domain not set yet                        */
    HN_ERR_UNSUPPORTED = -3, /* architecture / activation the kernels do not implement       */
    HN_ERR_HIP = -4,      /* a HIP runtime call failed                                       */
    HN_ERR_NOMEM = -5
};

/* activation kinds accepted by hn_load_weights (architectures.py:5-44 getActivationFunction): every name the
 * reference knows except 'relu_batchnorm' (it carries BatchNorm2d parameters and running statistics in the
 * state_dict); an unknown kind returns HN_ERR_UNSUPPORTED, mirroring the reference's NotImplementedError.
 * The piecewise-linear ones (0..2) take their slope from the blob (constant for relu / leakyrelu); 3..7 are
 * evaluated in fp32 in the kernels' epilogues: celu (alpha 1), tanh, gelu (erf form), tanhshrink, softplus
 * (beta 1, threshold 20). */
enum hn_act { HN_ACT_PRELU = 0, HN_ACT_RELU = 1, HN_ACT_LEAKYRELU = 2, HN_ACT_CELU = 3, HN_ACT_TANH = 4, HN_ACT_GELU = 5,
              HN_ACT_TANHSHRINK = 6, HN_ACT_SOFTPLUS = 7 };

/* Arithmetic of the UNet convolutions (hn_set_unet_precision).  Everything in HBM (activations, hidden state,
 * wavefield, residual), the 1x1 out-conv, the wavefield update and the spectral residual are fp32 in every mode.
 *   HN_PREC_FP32     every product in fp32 on the f32-input matrix core (default; the reference's arithmetic)
 *   HN_PREC_BF16X3   3-term bf16 split of both operands, 6 product terms, fp32 accumulate: fp32-accurate emulation
 *   HN_PREC_FP16     fp16 operands, fp32 accumulate: the "mixed fp16 UNet / fp32 spectral residual" configuration
 *   HN_PREC_BF16X2   2-term bf16 split, 3 product terms (~2^-16 relative, full fp32 exponent range)
 *   HN_PREC_FP32_VALU  fp32 on the vector ALU (direct convolution; A/B reference for the matrix-core kernels) */
enum hn_precision { HN_PREC_FP32 = 0, HN_PREC_BF16X3 = 1, HN_PREC_FP16 = 2, HN_PREC_BF16X2 = 3, HN_PREC_FP32_VALU = 4 };

/* Tuning knobs (hn_set_option).  Bit-exact ones -- the same kernels and summation order, only launched differently: LANES,
 * SIDE_STREAM, SPECTRAL_COLS (same butterflies, other memory access).  The others select a different kernel for the same
 * fp32 arithmetic and agree to fp32 rounding, like two fp32 implementations of the reference do: DEEP (other summation order,
 * 2e-6 * max), SPECTRAL_PFA and SPECTRAL_MIXED (FFT instead of the dense operator), SPECTRAL_RADIX16 (other butterfly order), DC_VALU. */
enum hn_option {
    HN_OPT_LANES = 0,        /* 1..8 sub-batches pipelined on internal streams (default 1; [measured, r5] 2 loses 3 % at 256^2 x 32 and 2 % at
                              * 256^2 x 64 -- one chain of 64 maps is the faster form since the r5 level-0 kernels --, +1 % at batch 128).
                              * Lane j of `lanes` takes samples [batch * j / lanes, batch * (j + 1) / lanes) (integer division); a call whose
                              * batch < 2 * lanes runs as ONE lane (with HN_EXP_GRAPH as set, but with event hand-overs: HN_OPT_SIDE_SYNC asks
                              * for the option to be 1).  Several lanes launch every kernel: HN_EXP_GRAPH does not apply to them */
    HN_OPT_SIDE_STREAM = 1,  /* conv_state kernels: 0 in line; on a library side stream released 1 after the last `down`,
                              * 2 level by level behind conv_signal, 3 behind the fused deep level               */
    HN_OPT_DEEP = 3,         /* the deep levels as one launch.  1: deepest level (32^2) + bottleneck in one per-sample LDS kernel (hn_deep.hip; 256^2 at
                              * depth 4).  2 (default): where the last encoder level is 64^2 (512^2) or the last two are 64^2 and 32^2 (256^2), those
                              * levels + the bottleneck as ONE launch with EIGHT workgroups per sample that exchange halo rows through flag-guarded
                              * global memory (hn_deepx.hip; batches up to 32 maps per call, every activation; fp32 arithmetic, which is what the 16-bit
                              * modes use below level 1 anyway -- they take this launch too), else as 1.  0: layer
                              * by layer.  Its waits are bounded like HN_OPT_SIDE_SYNC's and report through hn_check_async_errors                   */
    HN_OPT_SPECTRAL_PFA = 4, /* 0/1: prime-factor FFT for n = 3 * 2^k, 5 * 2^k, 7 * 2^k instead of the dense n x n operator (default 1;
                              * read by the next hn_set_domain)                                                     */
    HN_OPT_SPECTRAL_MIXED = 17, /* 0/1 (default 0): FFT for every other size n = P * 2^k, P odd >= 9 (2^k >= 16: all multiples of 16 that are neither a power
                              * of two nor taken by HN_OPT_SPECTRAL_PFA; with HN_OPT_SPECTRAL_PFA 0 also P = 3, 5, 7) instead of the dense n x n operator:
                              * P interleaved 2^k-point transforms in LDS and a direct P-point DFT across them (hn_spectral_line.hip).  Agrees with
                              * the dense operator to fp32 rounding, not bit for bit; read by the next hn_set_domain.  HN_CNT_SPECTRAL_ROUTE tells
                              * which route the current domain took                                                            */
    HN_OPT_F64_FFT = 18,     /* 0/1 (default 0; environment default HN_F64_FFT): the route of the float64 operator (hn_laplacian_f64, hn_residual_f64, hn_step_f64,
                              * both refine cycles).  0: the dense circulant kernel (24 n^3 flops per sample).  1: two line passes by FFT in double
                              * (hn_f64_fft.hip: n = P * 2^k, every legal size, a line in LDS), which agree with the dense kernel to float64 rounding
                              * (<= 2e-11 * max), not bit for bit.  Read by every float64 call, so it can be flipped between calls on one domain: each route
                              * keeps its own tables, built by its first call (not under stream capture), and flipping back gives the earlier bits.
                              * HN_CNT_F64_ROUTE tells which route the last call took.  [measured, profiles/f64_fft_bench.txt] the FFT
                              * route is faster at every measured size: 0.106 vs 0.311 ms at 256^2 x 32, 0.257 vs 1.100 at 512^2 x 16, 0.323 vs 2.360 at
                              * 1024^2 x 4, 0.470 vs 5.551 at 2048^2; it stays opt-in until the default is decided on those numbers */
    HN_OPT_SPECTRAL_RADIX16 = 5, /* 256-point lines: 0 the radix-4 kernels, 1 radix-16 columns + 8x4x8 rows (default), 2 radix-16 rows too */
    HN_OPT_DC_VALU = 6,      /* fp32 DoubleConvs of the largest level (W >= 256) on the packed vector FMA (every FMA useful, same peak as the
                              * fp32 MFMA, whose 3x3 packing fills 75 % of its slots): 0 none (matrix core); 1 inc and the decoder, 2 all three on the
                              * compiler-scheduled kernel (hn_dcv.hip); 3 inc and the decoder, 4 (default) all three on the hand-scheduled kernel
                              * (hn_dca.hip: all 8 mid channels per wavefront, LDS-direct staging; [measured, r5] +1 .. 3 % it/s over 1).  Smooth
                              * activations and unaligned tensors always take hn_dcv.hip                                          */
    HN_OPT_DC_PAIR = 12,     /* 0/1 (default 1): where inc and conv_signal_0 both run on hn_dca.hip they are ONE launch -- conv_signal's blocks wait, tile by
                              * tile, on a flag the inc blocks of the tiles they read publish (write-through stores, agent-scope flag).  The same launch
                              * eagerly, under stream capture (HN_OPT_GRAPH: the launch's epoch is derived on the device there) and in every pipeline
                              * lane.  Bit-identical to the two launches.
                              * ASSUMES that the workgroups of a launch are dispatched in index order (true of the hardware dispatcher; a tool that
                              * re-orders or caps dispatch must run with 0): a conv_signal block whose inputs have not arrived after ~2 M polls
                              * writes NaN into its tile AND raises the context's sticky device error (HN_ERR_STATE from this or the next hn_step) */
    HN_OPT_SIDE_SYNC = 13,   /* 0/1 (default 1): between the iterations of ONE hn_step call the side stream is joined -- and, at 256^2, released -- through
                              * device words that kernels of the main chain store / poll on their way (one thread each) instead of event packets,
                              * each of which holds the main stream for ~7 us; a call forks the side stream with one event and its LAST iteration uses events.
                              * hn_step's single-lane eager path -- HN_OPT_LANES 1, a call that replays no graph (HN_EXP_GRAPH 0, or a call that form
                              * stands down for), HN_PREC_FP32, HN_OPT_SIDE_STREAM 1, no st_hist (a state history reads the new states right behind
                              * every iteration); waits are bounded (2 s, then hn_step fails: the call in
                              * which a wait gave up returns HN_ERR_STATE if the error word is up by the time its launches are enqueued, else the next
                              * call does; hn_check_async_errors after a stream synchronise is the reliable test).
                              * The same option switches hn_train_grad's side stream (HN_OPT_TRAIN_OVERLAP 2) to device words (words 64 .. 160 of the
                              * context's 256 sync words; eager calls only) and then opens that side-stream window at every problem size instead of
                              * 200 k .. 1 M pixels; hn_train_grad reports a timed-out wait of an EARLIER call as HN_ERR_STATE at entry.
                              * Same kernels, same results; [measured, r5] +1 % it/s at 256^2 x 32, +8 % at batch 8.  A tool that runs ONE kernel at
                              * a time across all queues (counter collection: rocprofv3 --pmc) can starve such a wait: hn_create then defaults
                              * to 0 (ROCPROF_COUNTER_COLLECTION / ROCPROF_COUNTERS / ROCP_METRICS in the environment); any other such tool gets
                              * HN_ERR_STATE from hn_step after 2 s and must set HN_SIDE_SYNC=0                                              */
    HN_OPT_STATE_KERNEL = 14, /* 0/1 (default 1): the hidden-state DoubleConvs (10 -> 2 -> 2) of the levels at least 64 wide on the streaming kernel
                              * (hn_cs.hip: the tile's ten input planes through a ring of LDS-direct loads); 0: the general direct kernel.
                              * Bit-identical                                                                                          */
    HN_OPT_MC_STAGE = 19,    /* 0/1 (default 1): the fp32 matrix-core 8x8 stride-2 convolutions of the levels more than 32 outputs (down) / 64 inputs (up) wide
                              * and the 16-channel decoder DoubleConv of the levels at least 128 wide that run on the matrix core, with the input
                              * staging off the matrix pipe's critical path (the next chunk is committed to LDS behind the MFMAs of the current one,
                              * one barrier per chunk, no register copies, a prologue that loads before it plans; hn_mfma.hip: k_down_mfma_ring,
                              * k_up_mfma_ring, k_dc_mfma_s<.., RING>); 0: the kernels as they were.  The same MFMAs in the same order on every
                              * accumulator: bit-identical.  [measured, profiles/mc_stage_ab.txt] +2.1 % it/s at 256^2 x 32, +1.9 % at 512^2 x 16 */
    HN_OPT_MODULE_MC = 20,   /* 0/1 (default 0): hn_double_conv for (6,8), (8,8), (10,8), (16,8) and hn_conv8x8 run on the NETWORK's dispatch -- launch_dc8 /
                              * launch_down / launch_up with fragments packed from the call's weights as hn_load_weights packs a layer's -- instead of the direct
                              * kernels, so the precision mode, HN_OPT_DC_VALU and HN_OPT_MC_STAGE pick the kernel as they do in the network, at any H x W
                              * (see the sub-module entry points and hn_module_route).  0: every bit and every launch as before             */
    HN_OPT_HIST_COPY = 15,   /* 0 (default): hn_step's residual / wavefield histories are written in place of the copies (see hn_step); 1: every
                              * iteration works in the caller's wf / res and copies them into the history slots (A/B; bit-identical)       */
    HN_OPT_INC_SIGMA_MAP = 16, /* 0/1 (default 1): the sigma maps are constants of the domain and two of the six input channels of every UNet evaluation the solver
                              * makes (hybridnet.py:564-566), so their share of the input layer's first convolution is precomputed per domain (float64 on the
                              * host, at hn_load_weights / hn_set_domain) and the hand-scheduled input layer (HN_OPT_DC_VALU 3 / 4) convolves four
                              * channels, adding the map in the tiles near the border (it is zero elsewhere).  Agrees with 0 to fp32 rounding  */
    HN_OPT_SPECTRAL_COLS = 7, /* 256-point column pass: 0 the r2 kernel (16-byte global accesses), 1 (default) / 2: coalesced float4 row
                              * segments transposed through LDS, 16 / 32 columns per workgroup; 0, 1 and 2 give the same bits.  3: the staging
                              * of 1 around the row pass's 8 x 4 x 8 transform, 32 threads per column (k_spec8_cols_t: four wavefronts per
                              * SIMD instead of two): another factorisation, equal to the others within fp32 rounding, not bit for bit    */
    HN_OPT_TRAIN_FUSED = 10, /* hn_train_grad: sum of 1 (forward pass: an 8-channel DoubleConv is ONE launch of the fused matrix-core kernels of
                              * the inference path, which also store the pre-activation mid tensor to the tape; same tape within fp32
                              * rounding), 2 (backward pass: both backward-data convolutions of a big level's DoubleConv as one tiled
                              * launch; bit-identical gradients), 4 (the hidden-state DoubleConvs of all levels as one launch per
                              * direction instead of two; bit-identical), 16 (the backward-data pass of every 8-channel DoubleConv on the fp32 matrix
                              * core, k_dc_bwd_mfma_p: one launch, the g_z tile in LDS; the f32 matrix instruction is an exact fmaf chain in the vector
                              * kernels' order: bit-identical gradients at the training sizes) and 32 (with 4 and 16: conv_state's backward-data pass
                              * rides in the decoder's launch of the same level, k_dc_bwd_mfma_aux; d loss / d out is added up in one accumulator: fp32
                              * rounding); default 55, 0: every convolution as its own launch (round 3).  (Value 8 is a lab setting: the small
                              * levels' backward DoubleConvs on the tiled kernel; measured slower.)                                       */
    HN_OPT_TRAIN_OVERLAP = 11, /* hn_train_grad, backward pass: where the three weight-gradient launches of unrolled iteration t run.  0: in line on the
                              * caller's stream.  2 (default): on a library stream beside the backward chain of iteration t - 1 (two sets of gradient
                              * buffers) AND, where the chain is latency-bound (200 k .. 1 M pixels per call), with at most ~2 of their blocks per CU --
                              * each walks more tiles, the chain keeps half of every CU: 9.13 -> 8.77 ms at 96^2 x 32 -- and the forward sweep's
                              * hidden-state launch on that stream beside the decoder.  The cap changes how many partial sums a weight gradient is added
                              * up from: a fixed order (reproducible), not mode 0's.  (Value 1 is a lab setting: the side stream without
                              * the cap; bit-identical to 0 and measured equal to it.)                                                    */
    /* ---- laboratory knobs (same setter): implemented, tested bit-identical / equal within rounding, and MEASURED NOT TO HELP; they stay for A/B runs
     * and are not part of the supported surface (DESIGN_NOTEBOOK.md has the measurements) ---- */
    HN_EXP_GRAPH = 100,      /* 0: launch every kernel (default; measured 4 % faster); 1: replay one captured iteration per HIP graph
                              * launch; even n <= 64: n iterations per graph.  Bit-identical.  One lane only, and only in a call of at least
                              * 4 * n iterations (4 for the value 1): a shorter call launches every kernel, as 0 does.  With n > 1 a call
                              * replays floor(n_iter / n) graphs and launches the left-over iterations kernel by kernel, and it stands down
                              * altogether (every kernel launched) when the call has a res_hist, wf_hist or st_hist or while hn_profile_enable
                              * selects a kernel.  The side stream's kernels are part of the captured iteration under every HN_OPT_SIDE_STREAM
                              * policy.  A graph is captured once per set of (wf, res, states, k_sq, src, rmse_hist, src_batch, batch, precision,
                              * HN_OPT_SIDE_STREAM, HN_EXP_GRAPH) and kept (eight sets, least recently used first out) until the next hn_set_option, change of precision mode,
                              * hn_load_weights or hn_set_domain, each of which drops them all; HN_CNT_GRAPHS_CAPTURED counts
                              * the captures, so a call that should have replayed and could not shows up in the counters                  */
    HN_EXP_TRAIN_LANES = 101, /* hn_train_grad: 1 (default) the whole batch as one chain of launches; 2: the two halves of the batch as
                              * two chains on two streams.  Same gradient up to the order of the final sum over the halves; measured equal to 1 */
    HN_EXP_SPECTRAL_PLAIN = 102 /* 0 (default): the 256-point 8x4x8 row pass, the 256-point transposed column pass and both 512-point passes multiply and
                              * rotate complex numbers with the swap and the sign in the operand modifiers of the packed instructions; 1: the same
                              * kernel bodies instantiated on plain C++ helpers (kernel names with the suffix _plain).  Bit-identical
                              * (same products, same fused multiply-adds); for the bit-identity test and in-process A/B runs                 */
};
/* Diagnostics counters (hn_get_counter). */
enum hn_counter { HN_CNT_GRAPH_REPLAYS = 0,     /* hn_step iterations that ran as (part of) a graph replay (HN_EXP_GRAPH) */
                  HN_CNT_EAGER_ITERATIONS = 1,  /* hn_step iterations launched kernel by kernel; with several lanes one per iteration, not per lane.  Every
                                                 * iteration of every call counts in exactly one of the two */
                  HN_CNT_GRAPHS_CAPTURED = 2,   /* captures (one per new set of buffers and options, see HN_EXP_GRAPH) */
                  HN_CNT_STREAM_PROBES = 3,     /* reference-stream sets probed so far (see "side streams" in the conventions above) */
                  HN_CNT_SIDE_CANDIDATE = 4,    /* candidate (0 .. 3) hn_step's side stream was last picked from; -1 before the first pick */
                  HN_CNT_TRAIN_FWD_EVENTS = 5,  /* times hn_train_grad recorded the registered forward event (hn_train_set_forward_event): a caller compares the
                                                 * counter before and after a call to know whether event and table are valid for it (not under capture) */
                  HN_CNT_FLAG_SYNC_ITERATIONS = 6,  /* hn_step iterations whose side-stream hand-overs went through device words (HN_OPT_SIDE_SYNC): n_iter - 1 per
                                                 * eligible call (see HN_OPT_SIDE_SYNC), 0 with the option off, under stream capture and in a call that replays
                                                 * graphs, under counter collection, with HN_OPT_LANES > 1 (also where a small batch runs as one lane), with another
                                                 * HN_OPT_SIDE_STREAM policy than 1, in the 16-bit and HN_PREC_FP32_VALU modes, with a st_hist */
                  HN_CNT_SPECTRAL_ROUTE = 7,    /* not a count: the kernels the current domain's spectral operator runs on.  0 no domain, 1 power of two,
                                                 * 2 prime-factor (HN_OPT_SPECTRAL_PFA), 3 dense, 4 mixed (HN_OPT_SPECTRAL_MIXED),
                                                 * 5 rectangular (hn_set_domain_rect with h != w) */
                  HN_CNT_F64_ROUTE = 8 };       /* not a count: the route the last float64 call on this domain took (HN_OPT_F64_FFT).  0 none yet (reset by
                                                 * hn_set_domain / hn_set_domain_rect), 1 dense, 2 FFT */

#define HN_ABI_VERSION 7
int hn_abi_version(void);

/* Create / destroy a context on HIP device `device_id`. */
int hn_create(hn_ctx** out, int device_id);
void hn_destroy(hn_ctx* ctx);
const char* hn_last_error(const hn_ctx* ctx);

/* Number of fp32 values hn_load_weights expects for (features, depth, state_ch): the `f.*`
 * tensors of the checkpoint in state_dict order (architectures.py:317-388). */
size_t hn_weight_count(int features, int depth, int state_ch);

/* Upload the HybridNet parameters (HOST pointer; copied and re-packed, caller keeps `blob`).
 * Replaces: HybridNet.__init__ + load_state_dict (architectures.py:317-388).
 * Order of `blob`: inc.double_conv.{0.weight,0.bias,1.weight,2.weight,2.bias};
 *   for d in 0..depth-1: enc.d.conv_signal (5 tensors), enc.d.down.{weight,bias},
 *                        enc.d.conv_state (5 tensors);
 *   decode.0..depth (5 tensors each); up.0..depth-1 {weight,bias}; outc.conv.{weight,bias}.
 * Supported: features == 8, state_ch == 2, 1 <= depth <= 6, state_depth == depth. */
int hn_load_weights(hn_ctx* ctx, const float* blob, size_t n_floats, int features, int depth,
                    int state_ch, int act_kind);

/* Select the arithmetic of the UNet convolutions for every later call on this context (per context, not per
 * process: two contexts may differ).  The default is HN_PREC_FP32, or what the environment variable HN_UNET_IMPL
 * (fp32 | bf16x3 | fp16 | bf16x2 | valu) named when hn_create ran.  The reference has a single fp32 path
 * (architectures.py:439-465); the 16-bit modes are this library's extension (BASELINE.json configs[4]). */
int hn_set_unet_precision(hn_ctx* ctx, int precision);
int hn_get_unet_precision(const hn_ctx* ctx);
int hn_set_option(hn_ctx* ctx, int option, int value);
int64_t hn_get_counter(const hn_ctx* ctx, int counter);
/* Device-side waits of this library (HN_OPT_SIDE_SYNC, HN_OPT_DC_PAIR) are bounded and report through a sticky host-visible word; a call can only
 * see what is up by the time it returns, and the last hn_step of a solve has no successor.  HN_OK, or HN_ERR_STATE (with the message) if any wait
 * of any earlier call on this context gave up -- call it after synchronising the stream the work ran on.  No GPU work, no synchronisation. */
int hn_check_async_errors(hn_ctx* ctx);

/* Build the spectral-operator constants for an n x n domain (float64 on the host, fp32 on the
 * device): k grids, PML coefficients ax/bx/ay/by, sigma maps, FFT twiddles.
 * Replaces: FastLaplacianWithPML.init_variables / get_gamma_functions (spectral.py:267-363),
 * FourierDerivative k-grid (spectral.py:126-146), IterativeSolver.set_laplacian
 * (hybridnet.py:110-131).  n must be divisible by 2^depth (16 for the shipped net). */
int hn_set_domain(hn_ctx* ctx, int n, int pml, float sigma_max, float k);

/* ---- rectangular domains (added within ABI v7: a new entry point, nothing existing changes, so HN_ABI_VERSION stays 7) ----
 * hn_set_domain_rect: an h x w domain, h rows (the y axis, the first spatial index) by w columns (the x axis, the last index); tensors are
 * [B, C, h, w], contiguous.  The tables are the reference's formulas taken per axis (spectral.py:126-146, 298-363), each axis normalised by its own
 * length: sigma_x[i, j] = sigma_w[j], sigma_y[i, j] = sigma_h[i]; kx, ax, bx vary along the last axis (length w), ky, ay, by along the first (length h).
 * h and w must each satisfy what hn_set_domain asks of n: a multiple of 2^depth (16 for the shipped net) in [16, 2048] with 1 <= pml <= len / 2
 * (HN_ERR_ARG otherwise).  h == w IS hn_set_domain(ctx, h, ...): same routes, same tables, same bits from every entry point.
 * On a rectangular domain (h != w):
 *   - hn_state_len returns sum_d (h >> d) * (w >> d); the flat state is [B, 2, that], level 0 first, each level row-major; hn_get_sigmas writes [2, h, w];
 *     hn_get_counter(HN_CNT_SPECTRAL_ROUTE) returns 5;
 *   - hn_reserve, hn_get_sigmas, hn_laplacian, hn_residual, hn_rmse, hn_unet and hn_step work with the contracts they have on a square (hn_step: all four
 *     histories and rmse_hist, the overlap check, 4-byte-aligned pointers, n_iter in one call = the same iterations in several calls bit for bit) in
 *     HN_PREC_FP32 and HN_PREC_FP32_VALU.  The spectral residual runs by FFT on every legal length (each axis factored on its own as P * 2^k, P odd <= 127);
 *     the UNet runs layer by layer on the caller's stream, the histories are copied.  The workspace is sized from (h, w, batch), built by the first
 *     call or hn_reserve and freed by the next domain or weight load: a call that builds or grows it under stream capture returns HN_ERR_STATE with
 *     nothing enqueued; later calls are plain launches and capturable;
 *   - every other entry point that reads the domain returns HN_ERR_UNSUPPORTED, its message naming the rectangular domain, with nothing enqueued:
 *     hn_residual_vjp, the _f64 family, the GMRES family, hn_train_reserve / hn_train_grad, hn_step_vjp, hn_step_jvp, hn_stream_swap; so do hn_unet and
 *     hn_step in a 16-bit precision mode and hn_step with HN_OPT_LANES > 1.  HN_EXP_GRAPH, HN_OPT_SIDE_STREAM, HN_OPT_DEEP and HN_OPT_DC_PAIR have no
 *     effect.  Shape-free calls are unchanged (hn_stream_verdict, hn_adam_step, hn_rows_*, hn_double_conv, hn_conv8x8, hn_out_conv).
 * A later hn_set_domain or hn_set_domain_rect replaces the domain and frees what the previous one built. */
int hn_set_domain_rect(hn_ctx* ctx, int h, int w, int pml, float sigma_max, float k);

/* Copy the sigma maps [2, n, n] (sigma_x, sigma_y) to `out` (device). hybridnet.py:126-131. */
int hn_get_sigmas(hn_ctx* ctx, float* out, void* stream);

/* Total hidden-state length per channel, sum_d (n / 2^d)^2 (architectures.py:390-404). */
int64_t hn_state_len(const hn_ctx* ctx);

/* Pre-allocate the activation workspace for batches up to `max_batch` (optional; otherwise
 * grown by the first call, which then must not be under stream capture). */
int hn_reserve(hn_ctx* ctx, int max_batch);

/* out[B,2,n,n] = L(wf[B,2,n,n]), the spectral Laplacian with PML.
 * Replaces: IterativeSolver.apply_laplacian (hybridnet.py:540-542) +
 * fast_laplacian_with_pml (spectral.py:31-79). */
int hn_laplacian(hn_ctx* ctx, const float* wf, float* out, int batch, void* stream);

/* res[B,2,n,n] = L(wf) + k_sq * wf - src;  k_sq is [B,1,n,n]; src is [src_batch,2,n,n] with
 * src_batch == 1 (broadcast) or == batch.  Replaces get_residual (hybridnet.py:544-556). */
int hn_residual(hn_ctx* ctx, const float* wf, const float* k_sq, const float* src, int src_batch,
                float* res, int batch, void* stream);

/* out[B,2,n,n] = J^T g: the vector-Jacobian product of hn_residual with respect to the wavefield, i.e. the adjoint operator
 * L^H(g) + k_sq * g (real k_sq; L^H is the conjugate transpose of the spectral Laplacian with PML).  What torch.autograd
 * computes when the reference back-propagates through get_residual (hybridnet.py:544-556) in training_step (:385-413); also
 * the building block of adjoint-state / normal-equation solvers.  g must not alias out. */
int hn_residual_vjp(hn_ctx* ctx, const float* g, const float* k_sq, float* out, int batch, void* stream);

/* rmse[B] = sqrt(mean_{c,h,w} res^2).  Replaces test_loss_function (hybridnet.py:295-297). */
int hn_rmse(hn_ctx* ctx, const float* res, float* rmse, int batch, void* stream);

/* The same operator in float64, as an independent check of the fp32 residual: what the reference computes after solver.double()
 * (apply_laplacian / get_residual, hybridnet.py:540-556, on fast_laplacian_with_pml, spectral.py:31-79 run under .double(): the fp32 tables'
 * values, float64 arithmetic).  Two routes, each for every legal domain size, chosen per call by HN_OPT_F64_FFT: 0 (default) dense circulant derivative
 * operators on the f64 matrix instruction; 1 two line passes by FFT in double, one partial sum of squares per line (the rmse does not depend on the batch
 * on either route).  The routes agree to float64 rounding, not bit for bit; each builds its own tables (and, for an rmse-only call on the FFT route, an
 * intermediate field [B,2,n,n]) at its first call, under the capture rule below.
 * Shapes and layout as for hn_laplacian / hn_residual, all tensors doubles.  wf must not overlap out / res (HN_ERR_ARG).
 * hn_residual_f64: res[B,2,n,n] (may be NULL) and / or rmse[B] = sqrt(mean_{c,h,w} res^2) (may be NULL; not both, HN_ERR_ARG), the RMSE summed in a
 * fixed order (bit-reproducible).  The first call on a domain builds and uploads the float64 tables (freed by the next hn_set_domain / hn_destroy), and
 * an rmse call with a larger batch than any before grows a table of partial sums: such a call under stream capture returns HN_ERR_STATE before
 * enqueuing anything; once they exist the calls are capturable.  Plain launches on the caller's stream.  HN_ERR_STATE before hn_set_domain. */
int hn_laplacian_f64(hn_ctx* ctx, const double* wf, double* out, int batch, void* stream);
int hn_residual_f64(hn_ctx* ctx, const double* wf, const double* k_sq, const double* src, int src_batch,
                    double* res, double* rmse, int batch, void* stream);

/* ---- restarted GMRES on the same operator (added within ABI v7: a new entry point, nothing existing changes) ----
 * The reference's classical baseline is MATLAB's restarted gmres on the spectral PML operator (matlab/spectral_gmres_solver.m:86-115).
 * hn_gmres_cycle: ONE restart cycle of GMRES(restart) on A u = L(u) + k_sq * u (hn_residual with a zero source), for `batch` independent samples in
 * lock step: r = rhs - A x, v_0 = r / |r|; per inner step w = A v_k, two passes of classical Gram-Schmidt (H[:k+1, k] = h + h2), H[k+1, k] = |w|,
 * v_{k+1} = w / |w|; progressive Givens rotations per sample (double precision on the fp32 H column) with the residual estimate |g[j+1]| / sqrt(2 n^2).
 *   x        [B,2,n,n]  in: the iterate at the start of the cycle, out: the iterate after it (bit-for-bit untouched for a sample that starts below tol)
 *   k_sq     [B,1,n,n]; rhs [rhs_batch,2,n,n], rhs_batch in {1, batch}
 *   basis    [B, restart+1, 2*n*n]      caller-owned scratch; on return the orthonormal Arnoldi vectors of this cycle
 *   hess     [B, restart+1, restart, 2] caller-owned; on return the (re, im) Hessenberg matrix BEFORE the rotations
 *   rmse     [restart+1, B]             row 0: the TRUE residual RMSE of x at the start of the cycle (hybridnet.py:295-297 definition),
 *                                       row j: the Givens estimate after j inner iterations (repeated after the sample has stopped)
 *   k_used   [B] int32                  inner iterations whose basis vectors entered this sample's update (0 .. restart)
 * Per-sample stop: a sample whose row 0 is below tol gets k_used = 0 and its x is not written; otherwise k_used is the first j whose estimate is below
 * tol (restart if none is) and x += sum_{j < k_used} y_j v_j with the back-substituted y of exactly that truncation; the other samples' work goes on.
 * A breakdown (|w| = 0) divides by a clamp (1e-30), not by zero.  All sums have a fixed order (per-block partial sums in a library workspace, summed
 * in block order by their consumer; no float atomics): two calls on the same inputs give the same bits in every output, and a sample's results do
 * not depend on what shares the batch with it.  Everything is enqueued on `stream` with no host synchronisation; besides the operator an inner step
 * is five launches.  The workspace (partial sums, g, rotations, y, two dense fields) is sized from (batch, restart, n): a call that must create or
 * grow it under stream capture returns HN_ERR_STATE with nothing enqueued; later calls are plain launches and capturable.  hn_set_domain and
 * hn_destroy free it.  HN_ERR_ARG: restart outside [1, 64], batch < 1, rhs_batch not in {1, batch}, a NULL pointer, a field that is not 16-byte
 * aligned, any two arguments overlapping, no domain set. */
int hn_gmres_cycle(hn_ctx* ctx, float* x, const float* k_sq, const float* rhs, int rhs_batch, int batch, int restart, float tol,
                   float* basis, float* hess, float* rmse, int32_t* k_used, void* stream);

/* ---- GMRES to float64 accuracy (added within ABI v7: a new entry point, nothing existing changes) ----
 * One refinement step of restarted GMRES: the true residual and the update in float64, the restart cycle in fp32 (hn_gmres_cycle's kernels).
 * Classical iterative refinement with GMRES(restart) as the inner solver: res = A x - b by the float64 operator (hn_residual_f64's), s = its RMSE,
 * the fp32 cycle on the SCALED correction equation A d = -res / s from d = 0 (a right-hand side of RMSE 1, whatever the residual has shrunk to),
 * x += s * d in float64.  The operator of both precisions is the same one: the fp32 tables' values.
 *   x        [B,2,n,n] double  in/out: the iterate
 *   k_sq     [B,1,n,n] float, rhs [rhs_batch,2,n,n] float, rhs_batch in {1, batch}: up-cast exactly, as hn_step_f64 treats fp32 tables
 *   rmse64   [B] double        out: the TRUE float64 residual RMSE of x at the START of the call, bit for bit what hn_residual_f64 returns for
 *                              (x, double(k_sq), double(rhs)): the same launches, the same fixed-order sum
 *   basis, hess, rmse [restart+1,B], k_used [B]: as hn_gmres_cycle, for the fp32 cycle on the scaled correction equation, s = max(rmse64, 1e-300),
 *                              rhs fp32(-res / s) (a true division), started from d = 0 with the tolerance max(tol / s, inner_floor) on ITS
 *                              residual RMSE (rmse row 0 is about 1).  They equal, bit for bit, what hn_gmres_cycle returns for that right-hand
 *                              side from x = 0 with a tolerance of the same value.
 * then x += s * d in float64 (one rounding of the product and one of the sum per element).
 * Per-sample stop: a sample whose rmse64 < tol gets k_used = 0 and its x is not written (bit for bit); its rmse column repeats row 0.  The call that
 * finds every sample below tol is therefore the final true check and writes no x.  inner_floor bounds the accuracy asked of the fp32 cycle from below
 * (its estimate carries no information below about 1e-6 of the right-hand side).
 * Zero residual: s is the clamp, the scaled right-hand side is exactly zero, the sample counts as stopped for every tol and x is untouched; nothing
 * divides by zero.
 * No host synchronisation: everything is enqueued on `stream` -- one up-cast launch, the float64 operator with its RMSE, one launch that scales the
 * residual down and writes the per-sample tolerance and stop words, the cycle's launches, one update launch.  All sums have a fixed order, no float
 * atomics: two calls on equal inputs give equal bits in every output, and a sample's results do not depend on its batch mates.
 * Workspace: the float64 copies of k_sq and rhs, one float64 residual field, the fp32 scaled right-hand side and correction, two words per sample,
 * plus hn_gmres_cycle's workspace and hn_residual_f64's tables, sized from (batch, restart, n) and freed by hn_set_domain / hn_destroy.  A call that
 * must create or grow any of them under stream capture returns HN_ERR_STATE with nothing enqueued; later calls are plain launches and capturable.
 * HN_ERR_ARG: restart outside [1, 64], batch < 1, rhs_batch not in {1, batch}, a NULL pointer, x / k_sq / rhs / basis not 16-byte aligned, tol or
 * inner_floor NaN or negative, any two arguments overlapping (x included).  HN_ERR_STATE before hn_set_domain. */
int hn_gmres_refine_cycle(hn_ctx* ctx, double* x, const float* k_sq, const float* rhs, int rhs_batch, int batch, int restart,
                          double tol, float inner_floor, float* basis, float* hess, float* rmse, int32_t* k_used, double* rmse64,
                          void* stream);

/* ---- flexible GMRES, preconditioned by the learned iteration (added within ABI v7: new entry points, nothing existing changes) ----
 * hn_fgmres_cycle is hn_gmres_cycle as a FLEXIBLE restart cycle (FGMRES, Saad 1993) with the learned solver as a right preconditioner that may
 * change from step to step and be nonlinear.  With m = precond_iters and alpha = precond_scale, inner step k computes z_k = M(v_k):
 *   m >= 1: the learned solve of A z = alpha v_k from rest on a library workspace -- src = alpha * v_k (one fp32 multiply per element), wf = 0,
 *           states = 0, res = 0 - src, then exactly the launches of hn_step(wf, res, states, k_sq, src, src_batch = batch, batch, n_iter = m, no
 *           histories) on `stream` (the context's precision mode and options apply as to any hn_step), z_k = wf / alpha (a true division);
 *   m == 0: z_k = v_k, copied exactly: x, basis, hess, rmse and k_used then equal hn_gmres_cycle's bit for bit and zbasis[:, j] == basis[:, j].
 * w = A z_k is the operator hn_gmres_cycle applies (not the step's last residual); the two Gram-Schmidt passes, the Hessenberg column, the rotations,
 * rmse, the per-sample stop and v_{k+1} = w / |w| are unchanged and work on `basis`; the update is x += sum_{j < k_used} y_j z_j.
 *   zbasis   [B, restart, 2*n*n]  caller-owned scratch like basis; on return the z_j of this cycle
 * Everything else as hn_gmres_cycle: a sample below tol at the start is untouched bit for bit, fixed-order sums, no float atomics, two calls on equal
 * inputs on a context with equal options give equal bits.  In exact arithmetic the residual estimate is the true residual of the truncated iterate
 * whatever M is (A Z_k = V_{k+1} H_k holds by construction).
 * hn_fgmres_refine_cycle is hn_gmres_refine_cycle with this cycle inside: the up-cast, the float64 operator, the scaled right-hand side, the float64
 * update, the per-sample tolerance and the stop words are the same launches in the same order, rmse64 is bit for bit hn_residual_f64's, and with m == 0
 * every output equals hn_gmres_refine_cycle's bit for bit.
 * Workspace: src, wf, res [B][2 n^2] and the hidden states [B][2][hn_state_len] beside hn_gmres_cycle's, built by the first call with m >= 1, grown by
 * a larger batch, freed by hn_set_domain, hn_load_weights and hn_destroy.
 * NOT capturable: under stream capture both return HN_ERR_STATE before enqueuing anything (hn_step's first call on a stream probes and synchronises).
 * For the same reason the FIRST call with precond_iters >= 1 on a stream blocks the host once, inside the first inner step (behind the launches
 * enqueued up to there), as a first hn_step on that stream would; later calls on it enqueue without a host synchronisation.  What hn_step reports
 * from inside the cycle comes back under this entry point's name.
 * HN_ERR_ARG: everything hn_gmres_cycle / hn_gmres_refine_cycle refuse, precond_iters < 0, precond_scale not finite or <= 0, zbasis NULL, not 16-byte
 * aligned or overlapping any other argument, and what hn_step refuses (a domain the network's depth does not divide).  HN_ERR_STATE before
 * hn_set_domain, and before hn_load_weights when precond_iters >= 1.  A refused call has enqueued nothing. */
int hn_fgmres_cycle(hn_ctx* ctx, float* x, const float* k_sq, const float* rhs, int rhs_batch, int batch, int restart, float tol,
                    int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess, float* rmse, int32_t* k_used,
                    void* stream);
int hn_fgmres_refine_cycle(hn_ctx* ctx, double* x, const float* k_sq, const float* rhs, int rhs_batch, int batch, int restart,
                           double tol, float inner_floor, int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess,
                           float* rmse, int32_t* k_used, double* rmse64, void* stream);

/* ---- adjoint-state gradients of a converged solve (added within ABI v7: new entry points, nothing existing changes; square domains, fp32) ----
 * With A u = src (A u = L(u) + k_sq * u), a real loss J(u) and its cotangent g = dJ/du (two real planes, g = dJ/du_re + i dJ/du_im), the adjoint
 * state is the solution of A^H lambda = g, A^H the conjugate transpose hn_residual_vjp applies.  From dJ = Re <g, du> and A du = dsrc - dk_sq * u:
 *   dJ/dsrc  = lambda                              (two real planes again)
 *   dJ/dk_sq = -Re(conj(lambda) * u) = -(lambda_re u_re + lambda_im u_im)
 * and, with k_sq = (omega / sos)^2, dJ/dsos = dJ/dk_sq * (-2 omega^2 / sos^3).  One extra linear solve and a pointwise product, whatever converged u.
 *
 * hn_fgmres_adjoint_cycle is hn_fgmres_cycle on the system A^H x = rhs: the same arguments, stop rule, outputs, workspaces and refusals (HN_ERR_UNSUPPORTED
 * on a rectangular domain), with these differences:
 *   - the operator of the start residual rhs - A^H x and of every inner step is A^H, on the route the domain's forward operator takes (power of two,
 *     prime-factor, mixed, dense);
 *   - precond_iters == 0: plain restarted GMRES on A^H, zbasis[:, j] == basis[:, j] bit for bit;
 *   - precond_iters >= 1: the learned network approximates A^-1, not A^-H.  Per axis the PML operator is (1/gamma) d (1/gamma) d with
 *     gamma = 1 + i sigma / k, so that W A is complex-symmetric up to the discretisation for W = diag(gamma_y[i] * gamma_x[j]): A^T ~ W A W^-1 and
 *     A^-H v ~ conj(W * A^-1 (conj(v) / W)).  Inner step k therefore runs the SAME learned solve as hn_fgmres_cycle on
 *       src = alpha * (conj(v_k) * Winv)     re = vr Wr' + vi Wi',  im = vr Wi' - vi Wr'   (Winv = Wr' + i Wi'; fp32 product sums, then one multiply)
 *       wf = 0, states = 0, res = 0 - src, hn_step's launches for precond_iters iterations,
 *       z_k = conj(W * wf) / alpha           re = (Wr fr - Wi fi) / alpha,  im = (0 - (Wr fi + Wi fr)) / alpha   (a true division)
 *     W and Winv = 1 / W are tables of the domain: gamma in double from the fp32 value of sigma (what hn_get_sigmas returns) and k, the product
 *     gamma_y[i] gamma_x[j] and its reciprocal in double, each rounded once to fp32.  They are built by the first call with precond_iters >= 1 on a
 *     domain (one allocation of 4 n^2 floats, a blocking copy) and freed by hn_set_domain / hn_destroy.
 * The preconditioner only has to be approximate: A^H Z_k = V_{k+1} H_k holds by construction, so the residual estimate stays that of the truncated
 * iterate.  Fixed-order sums, no float atomics: two calls on equal inputs give equal bits, and a sample's bits do not depend on its batch mates.
 * NOT capturable, like hn_fgmres_cycle, and the first call with precond_iters >= 1 on a stream blocks the host once. */
int hn_fgmres_adjoint_cycle(hn_ctx* ctx, float* x, const float* k_sq, const float* rhs, int rhs_batch, int batch, int restart, float tol,
                            int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess, float* rmse, int32_t* k_used,
                            void* stream);
/* The pointwise half of the adjoint-state gradient, one launch, no atomics, nothing synchronised:
 *   lambda, u [B,2,n,n]   the adjoint state and the wavefield
 *   g_k_sq   [B,1,n,n]    out: -(lambda_re * u_re + lambda_im * u_im)
 *   g_src    [src_batch,2,n,n] or NULL   out: lambda (src_batch == batch), or its sum over the batch in sample order (src_batch == 1: the source
 *                         every sample shared)
 * HN_ERR_ARG: a NULL pointer but g_src, batch < 1, src_batch not in {1, batch}, a pointer that is not 16-byte aligned, an output overlapping any other
 * argument (lambda may equal u).  HN_ERR_STATE before hn_set_domain, HN_ERR_UNSUPPORTED on a rectangular domain. */
int hn_adjoint_grad(hn_ctx* ctx, const float* lambda, const float* u, int src_batch, int batch, float* g_k_sq, float* g_src, void* stream);

/* d[B,2,n,n] = HybridNet(in6[B,6,n,n]); the hidden states are read from `states_in` and the new
 * ones written to `states_out`, both in the reference's flat layout [B, 2, hn_state_len()]
 * (architectures.py:419-437).  states_out and d_out must not overlap each other, states_in or in6 -- states_out is written level by level while
 * later kernels still read states_in, so a partial overlap is as wrong as equal pointers: HN_ERR_ARG "hn_unet: <a> overlaps <b>", nothing enqueued.
 * Any 4-byte-aligned pointers (see "alignment and overlap" above for what a pointer off a 16-byte boundary costs).
 * Replaces HybridNet.forward + EncoderBlock.forward (architectures.py:439-465, 240-252). */
int hn_unet(hn_ctx* ctx, const float* in6, const float* states_in, float* states_out, float* d_out,
            int batch, void* stream);

/* ---- the solver loop in float64 (added within ABI v7: new entry points, nothing existing changes) ----
 * hn_unet_f64: d[B,2,n,n] = HybridNet(in6[B,6,n,n]) in float64: the reference after solver.double() (architectures.py:439-465, 240-252).  Layout of
 * hn_unet, every tensor double; no two tensors may overlap unless both are only read (HN_ERR_ARG).  Weights: the fp32 values of the last
 * hn_load_weights up-cast exactly (what .double() does to the parameters); every activation kind is evaluated in double (erf gelu, softplus with
 * threshold 20, celu with alpha 1, leakyrelu with the double 0.01).  The reference's layers one by one, fixed summation order: bit-reproducible.
 * hn_step_f64: n_iter iterations of single_step (hybridnet.py:558-584) in float64,
 *   d = HybridNet(cat[wf, 1e3*res, sigmas]);  wf = d/1e3 + wf;  res = L(wf) + k_sq*wf - src   (the residual of hn_residual_f64),
 * arguments as hn_step, every tensor double, the sigma channels the fp32 table values up-cast; histories optional (NULL), rmse_hist[n_iter,B] from
 * hn_residual_f64's fixed-order sums.  wf, res, states are updated in place; no tensor may overlap another unless both are only read (HN_ERR_ARG).
 * Both: the up-cast weights, a float64 workspace (320 n^2 bytes per sample) and a second state buffer are built by the first call and grown by a
 * larger batch, and freed by the next hn_load_weights / hn_set_domain / hn_destroy; such a first or growing call under stream capture returns
 * HN_ERR_STATE before enqueuing anything (hn_step_f64 also where hn_residual_f64 would), later calls are plain launches on the caller's stream and
 * capturable.  HN_ERR_STATE before hn_load_weights / hn_set_domain.  A reference to measure the fp32 / fp16 / bf16 modes against, not a fast path. */
int hn_unet_f64(hn_ctx* ctx, const double* in6, const double* states_in, double* states_out, double* d_out, int batch, void* stream);
int hn_step_f64(hn_ctx* ctx, double* wf, double* res, double* states, const double* k_sq, const double* src, int src_batch,
                int batch, int n_iter, double* res_hist, double* wf_hist, double* st_hist, double* rmse_hist, void* stream);

/* The UNet's sub-modules on their own -- what DoubleConv.forward (architectures.py:83-84), the 8x8 stride-2 convolution /
 * transposed convolution of an EncoderBlock / the decoder (:209-211, :375-382, as called in EncoderBlock.forward :252 and
 * HybridNet.forward :456) and OutConv.forward (:57-60) compute, for the channel shapes the UNet is made of.  Utility
 * entry points: the weights come as HOST pointers in PyTorch layout and are re-packed and uploaded by every call (the
 * solver never uses them; hn_unet / hn_step run the whole network from the blob of hn_load_weights).  Tensors are
 * device pointers, NCHW fp32; no domain or network needs to be loaded.
 *   hn_double_conv  x[B,cin,H,W] -> out[B,cout,H,W];  (cin, cout) in {(6,8), (8,8), (10,8), (16,8), (10,2)}, mid = cout channels;
 *                   weights = conv1.weight [cout,cin,3,3], conv1.bias [cout], slope [1] (PReLU weight, or the constant slope of
 *                   relu / leakyrelu; ignored by the smooth activations), conv2.weight [cout,cout,3,3], conv2.bias [cout], concatenated
 *   hn_conv8x8      transposed = 0: Conv2d(8, 8, 8, stride 2, padding 3), x[B,8,H,W] -> out[B,8,H/2,W/2] (H, W even), weights =
 *                   weight [8,8,8,8] (out, in, kh, kw), bias [8];  transposed = 1: ConvTranspose2d(8, 8, 8, stride 2, padding 3),
 *                   x[B,8,H,W] -> out[B,8,2H,2W], weight [8,8,8,8] (in, out, kh, kw), bias [8]
 *   hn_out_conv     Conv2d(8, 2, 1): x[B,8,H,W] -> out[B,2,H,W], weights = weight [2,8], bias [2]
 * By default (HN_OPT_MODULE_MC 0) always the direct fp32 kernels (those of HN_PREC_FP32_VALU), whatever the context's precision mode; any H, W >= 1.  Refusals enqueue nothing and leave
 * `out` untouched: HN_ERR_UNSUPPORTED for another (cin, cout), an act_kind outside enum hn_act and an odd H or W of the stride-2 form; HN_ERR_ARG for a
 * NULL pointer or a non-positive batch, H or W.
 * HN_OPT_MODULE_MC 1: hn_double_conv with cout = 8 and hn_conv8x8 take the network's own dispatch instead, on temporary fragments packed from the call's
 * weights exactly as hn_load_weights packs a layer's (they live until the stream has been synchronised, like the direct path's weights): launch_dc8 as
 * the input layer (6), the bottleneck (8), conv_signal (10) or a decoder (16) with every input scale 1, launch_down / launch_up without accumulation.  The
 * precision mode, HN_OPT_DC_VALU and HN_OPT_MC_STAGE then select the kernel as in the network (hn_module_route names it); HN_PREC_FP32_VALU and (10,2)
 * keep the direct kernel (k_conv_state reads its weights as offsets into the loaded blob).  The input-layer instance of hn_dca.hip needs the
 * 1e3 scale on the residual channels and is NOT reachable this way: with HN_OPT_DC_VALU 3 / 4 a (6,8) call runs on hn_dcv.hip.  hn_dca.hip also needs a
 * context with weights loaded (its zero page).  Refusals and their messages are the same under either value. */
/* Kernel instances of that dispatch (hn_mfma.hip unless named otherwise), as hn_module_route reports them */
enum hn_route {
    HN_ROUTE_DIRECT = 0,            /* the direct fp32 kernels of hn_unet.hip: HN_OPT_MODULE_MC 0, HN_PREC_FP32_VALU, (10,2) */
    HN_ROUTE_DC_ASM = 1,            /* hn_dca.hip (HN_OPT_DC_VALU 3 / 4: W >= 256, W % 4 == 0, 16-byte aligned planes, piecewise-linear activation) */
    HN_ROUTE_DC_VALU = 2,           /* hn_dcv.hip (HN_OPT_DC_VALU 1 .. 4: W >= 256, even W) */
    HN_ROUTE_K_DC_MFMA_S = 3,       /* k_dc_mfma_s: 16 x 64 strips, even W >= 128 */
    HN_ROUTE_K_DC_MFMA_S_GEN = 4,   /*   ... with the general epilogue (smooth activations, every precision mode) */
    HN_ROUTE_K_DC_MFMA_S_RING = 5,  /*   ... the 16-channel decoder with HN_OPT_MC_STAGE 1 */
    HN_ROUTE_K_DC_MFMA_P_32 = 6,    /* k_dc_mfma_p<8, 32>: even 16 < W < 128 (the smooth activations' GEN instance has the same code, as below) */
    HN_ROUTE_K_DC_MFMA_P_16 = 7,    /* k_dc_mfma_p<8, 16>: even W <= 16 */
    HN_ROUTE_K_DC_MFMA_64 = 8,      /* k_dc_mfma<64>: odd W > 32, 16-row tiles (the any-shape kernel) */
    HN_ROUTE_K_DC_MFMA_32 = 9,      /* k_dc_mfma<32>: odd 16 < W <= 32 */
    HN_ROUTE_K_DC_MFMA_16 = 10,     /* k_dc_mfma<16>: odd W <= 16 */
    HN_ROUTE_K_DC_X16_BF16X3 = 11,  /* k_dc_x16<SplitBf16, .., 8>: 8 x 64 strips, even W >= 128, piecewise-linear activation (as the next two) */
    HN_ROUTE_K_DC_X16_FP16 = 12,    /* k_dc_x16<HalfF16>: 16 x 64 strips */
    HN_ROUTE_K_DC_X16_BF16X2 = 13,  /* k_dc_x16<SplitBf16x2> */
    HN_ROUTE_DOWN_64 = 14,          /* k_down_mfma<4>: 16 rows x 64 outputs, Wout > 64 */
    HN_ROUTE_DOWN_32 = 15,          /* k_down_mfma<2>: 32 < Wout <= 64 */
    HN_ROUTE_DOWN_16 = 16,          /* k_down_mfma<1>: Wout <= 32 */
    HN_ROUTE_DOWN_RING_64 = 17,     /* k_down_mfma_ring<4> (HN_OPT_MC_STAGE 1) */
    HN_ROUTE_DOWN_RING_32 = 18,     /* k_down_mfma_ring<2> */
    HN_ROUTE_DOWN_X16 = 19,         /* k_down_x16 (fp16, bf16x2): 16 x 16 outputs, Wout >= 64 */
    HN_ROUTE_UP_2_11 = 20,          /* k_up_mfma<2, 11>: 22 window rows x 32 input columns, Win > 64 */
    HN_ROUTE_UP_RING = 21,          /* k_up_mfma_ring<2, 11> (HN_OPT_MC_STAGE 1) */
    HN_ROUTE_UP_1_5 = 22,           /* k_up_mfma<1, 5, true>: 20 window rows x 16 input columns, Win <= 64 */
    HN_ROUTE_UP_X16 = 23            /* k_up_x16 (the three 16-bit modes): 20 window rows x 16 input columns, Win >= 64 */
};
/* The instance (enum hn_route) that hn_double_conv (op 0: a piecewise-linear activation, op 3: a smooth one; cin 6, 8, 10 or 16, cout 8) or hn_conv8x8
 * (op 1: stride 2, op 2: transposed; cin 8) would launch NOW for an h x w input of 16-byte aligned, densely packed planes: a pure function of the
 * context's precision mode and options and the shape.  Nothing is enqueued.  HN_ERR_ARG for another op, cin or a non-positive h, w (op 1: odd h, w). */
int hn_module_route(hn_ctx* ctx, int op, int cin, int h, int w);
int hn_double_conv(hn_ctx* ctx, const float* x, int cin, int cout, const float* weights_host, int act_kind, float* out,
                   int batch, int h, int w, void* stream);
int hn_conv8x8(hn_ctx* ctx, const float* x, const float* weights_host, int transposed, float* out, int batch, int h, int w,
               void* stream);
int hn_out_conv(hn_ctx* ctx, const float* x, const float* weights_host, float* out, int batch, int h, int w, void* stream);

/* n_iter fused solver iterations (hybridnet.py:558-584 single_step, looped as in
 * forward :654-697 / n_steps :586-623):
 *     d = HybridNet(cat[wf, 1e3*res, sigmas]); wf += d/1e3; res = L(wf) + k_sq*wf - src
 * wf, res and states (flat layout) are updated IN PLACE.
 * Optional outputs (NULL to skip):
 *     res_hist  [n_iter, B, 2, n, n]  residual after every iteration (the reference keeps them all)
 *     wf_hist   [n_iter, B, 2, n, n]  wavefield after every iteration (return_wavefields=True)
 *     st_hist   [n_iter, B, 2, L]     flat hidden state after every iteration (return_states=True)
 *     rmse_hist [n_iter, B]           per-sample residual RMSE after every iteration
 * Histories cost no copies (v7): the residual / wavefield of iteration `it` is WRITTEN into slot `it` of res_hist / wf_hist by the kernels
 * that compute it and read there by iteration it + 1 -- the reference keeps every residual for free too (it appends tensors, :676-697);
 * wf and res receive the last slot with one device-to-device copy per call.  With captured iterations (HN_EXP_GRAPH), several lanes or
 * HN_OPT_HIST_COPY 1 the r1 - r6 form (in place + one copy per iteration and history) runs.
 * Overlap: no tensor of the call that is written (wf, res, states and the four histories) may overlap any other; k_sq and src, which are only read,
 * may share memory.  HN_ERR_ARG "hn_step: <a> overlaps <b>" with nothing enqueued, in every form of the loop (zero-copy, HN_OPT_HIST_COPY 1, lanes,
 * captured iterations).  In particular wf / res may not be a view INTO their own history -- slot j > 0, or a view shifted against the slots: a later
 * iteration would overwrite it while the history still needs it, whichever form runs.  ONE form is tolerated: res_hist == res and / or wf_hist == wf
 * (equal pointers: the live buffer IS slot 0).  The copying form then runs; slots 1 .. n_iter - 1, wf, res and states are bit for bit those of a call
 * on separate buffers, and slot 0, being the live buffer, ends up holding the last iteration's value.
 * Alignment: any 4-byte-aligned pointers (see "alignment and overlap" above). */
int hn_step(hn_ctx* ctx, float* wf, float* res, float* states, const float* k_sq, const float* src,
            int src_batch, int batch, int n_iter, float* res_hist, float* wf_hist, float* st_hist,
            float* rmse_hist, void* stream);

/* ---- absorbing media: a complex k_sq (an extension like the rectangular domains; the reference's Python side has no counterpart, its MATLAB side
 * carries skull absorption in matlab/skull2medium.m).  The three entry points below take the medium as two real planes and evaluate
 *     res = L(wf) + (k_sq + i * k_sq_im) * wf - src:   re += k_sq * wf_re - k_sq_im * wf_im,   im += k_sq * wf_im + k_sq_im * wf_re.
 * Sign: the PML stretches with gamma = 1 + i sigma / k, so outgoing waves are e^{+ikx} and a medium ABSORBS for Im(k~) > 0.  With k~ = omega / c + i alpha
 * (alpha in nepers per grid point): k_sq = (omega / c)^2 - alpha^2, k_sq_im = 2 (omega / c) alpha >= 0.  A negative k_sq_im amplifies; it is accepted.
 * k_sq_im: fp32 [B,1,h,w], read only, any sign; NULL returns HN_ERR_ARG with a message that names the lossless sibling.  Its alignment and overlap rules
 * are those k_sq has in the sibling call, and it may overlap nothing that is written.  The UNet never sees k_sq (its six input channels are the
 * wavefield, 1e3 * residual and the two sigma maps), so absorption enters the residual alone.
 * Route: both line passes run on the general LDS-line kernel of the rectangular domains (any length P * 2^k), the row pass with the complex term.  On a
 * rectangular domain the tables exist; on a SQUARE domain they are built at the latest by the first lossy call on that domain -- which, where it has
 * them to build (every route but HN_OPT_SPECTRAL_MIXED's, whose own tables they are), must not be under stream capture: HN_ERR_STATE, nothing
 * enqueued -- kept until hn_set_domain / hn_set_domain_rect / hn_destroy, and change nothing of the lossless entry
 * points: hn_residual, hn_step and the cycles keep their kernels and their bits.  With k_sq_im = 0 the results agree with the lossless siblings to fp32
 * rounding, not bit for bit (another factorisation of the transforms).
 * Adjoint-state gradients of a converged lossy solve have the chain the lossless operator has: hn_residual_vjp_lossy (A^H g), hn_fgmres_adjoint_cycle_lossy
 * (A^H lambda = g) and hn_adjoint_grad_lossy (dJ/dk_sq, dJ/dk_sq_im, dJ/dsrc), further down.
 * The float64 half -- the residual check and GMRES to float64 accuracy -- is hn_residual_f64_lossy and hn_fgmres_refine_cycle_lossy, further down.
 * No entry point exists for: gradients through the solver loop (a lossy hn_step_vjp / hn_step_jvp), a lossy hn_step_f64, training. */

/* hn_residual with the complex pointwise term; every legal square size and every rectangular domain.  HN_ERR_ARG "hn_residual_lossy: k_sq_im overlaps res". */
int hn_residual_lossy(hn_ctx* ctx, const float* wf, const float* k_sq, const float* k_sq_im, const float* src, int src_batch, float* res, int batch,
                      void* stream);

/* hn_step on the lossy residual: per iteration exactly the UNet launches of hn_step, then the lossy spectral pair.  Arguments, in-place updates, the four
 * histories and rmse_hist mean what they mean in hn_step; k_sq_im joins k_sq and src as a read-only tensor of the overlap rule ("hn_step_lossy: <a>
 * overlaps <b>").  Square domains: every UNet precision mode; rectangular domains: the two fp32 modes, as hn_step.  Runs eagerly on one lane:
 * HN_OPT_LANES > 1 returns HN_ERR_UNSUPPORTED, HN_EXP_GRAPH is ignored. */
int hn_step_lossy(hn_ctx* ctx, float* wf, float* res, float* states, const float* k_sq, const float* k_sq_im, const float* src, int src_batch, int batch,
                  int n_iter, float* res_hist, float* wf_hist, float* st_hist, float* rmse_hist, void* stream);

/* hn_fgmres_cycle with the lossy operator in both places, w = A z and the true residual of row 0, and precond_iters iterations of hn_step_lossy on
 * A z = precond_scale * v as the preconditioner; precond_iters = 0 is plain restarted GMRES on the lossy operator.  Square domains only
 * (HN_ERR_UNSUPPORTED on a rectangular one).  Workspaces, the capture refusal and every argument check are hn_fgmres_cycle's; k_sq_im must be 16-byte
 * aligned and overlap no other argument, as k_sq. */
int hn_fgmres_cycle_lossy(hn_ctx* ctx, float* x, const float* k_sq, const float* k_sq_im, const float* rhs, int rhs_batch, int batch, int restart,
                          float tol, int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess, float* rmse, int32_t* k_used,
                          void* stream);

/* ---- heterogeneous density (added within ABI v7: new entry points, nothing existing changes) ----
 * matlab/skull2medium.m produces three maps, sound speed, absorption and density; this is the third.  With the PML stretch gamma = 1 + i sigma / k the
 * reference expands each axis of (1/gamma) d((1/gamma) du) as a du + b d2u, b = 1 / gamma^2, a = -gamma' / gamma^3.  Variable density in the same form:
 *     rho (1/gamma) d( (1/rho) (1/gamma) du ) = a du + b d2u - b q du,     q = d ln rho  (real, per axis, per pixel)
 *     A_rho u = L(u) - b_x q_x d_x u - b_y q_y d_y u + (k_sq + i k_sq_im) u
 * with d_x, d_y the Fourier derivatives and b_x, b_y the tables L itself uses.  This is the EXPANDED form, not the conservative discretisation
 * rho div((1/rho) grad u): products alias, and the two differ by 1-2 % for a smooth u and by O(1) for white noise.  Only ratios of rho matter.  A jump
 * in rho makes q ring; smooth the map as k-Wave users do.
 * rho_grad: fp32 [B,2,h,w], read only.  Plane 0 is q_x = d ln rho / dx, x the LAST index (length w, the axis of sigma_x); plane 1 is q_y, along the
 * first spatial index (length h).  Units: per grid point.  The library takes any gradient the caller prefers (helmnet_amd.density has the spectral
 * one).  NULL returns HN_ERR_ARG with a message that names the constant-density siblings.  k_sq_im MAY be NULL here: a lossless medium, the plane is not
 * read.  The UNet never sees the medium, so density enters the residual alone.
 * Route: the LDS-line kernel of the lossy operator, on its tables and under its capture rule (a square domain's are built at the latest by the first
 * lossy or variable-density call, which must not be under stream capture: HN_ERR_STATE, nothing enqueued).  Each pass reads its plane of rho_grad at the
 * element it stores and multiplies the first derivative with a - q b: one more fp32 plane read per pass, no further LDS, no further transform.
 * Nothing of the other entry points changes: they keep their kernels and their bits.  With rho_grad = 0 the results agree with the lossy (k_sq_im
 * NULL: the lossless) siblings to fp32 rounding.
 * [measured, MI355X, profiles/density_bench.txt] hn_residual_medium / hn_residual_lossy, alternating in one process: 1.060 at 256^2 x 32, 1.108 at
 * 512^2 x 16, 1.070 at 400^2 x 16 (from the traffic alone, 8 more bytes on about 56 per pixel: at most 1.14); one hn_step_medium iteration /
 * one hn_step_lossy iteration 1.023, 1.018, 1.019.
 * The adjoint of A_rho and the adjoint-state gradients of a converged solve are further down: hn_residual_vjp_medium (A_rho^H g),
 * hn_fgmres_adjoint_cycle_medium (A_rho^H lambda = g) and hn_adjoint_grad_medium (dJ/dk_sq, dJ/dk_sq_im, dJ/dq, dJ/dsrc).
 * No entry point exists for: anything float64, gradients through the loop, training, the stream of maps (hn_stream_swap). */

/* hn_residual_lossy with the density term; every legal square size and every rectangular domain.  rho_grad and k_sq_im may overlap nothing written
 * ("hn_residual_medium: rho_grad overlaps res"); 4-byte alignment suffices. */
int hn_residual_medium(hn_ctx* ctx, const float* wf, const float* k_sq, const float* k_sq_im, const float* rho_grad, const float* src, int src_batch,
                       float* res, int batch, void* stream);

/* hn_step_lossy on the variable-density residual: per iteration exactly the UNet launches of hn_step, then the density pair.  Histories, rmse_hist,
 * precision modes, the one lane (HN_OPT_LANES > 1: HN_ERR_UNSUPPORTED) and the overlap rule are hn_step_lossy's, rho_grad one more read-only tensor.
 * n_iter iterations in one call equal the same iterations in several calls bit for bit. */
int hn_step_medium(hn_ctx* ctx, float* wf, float* res, float* states, const float* k_sq, const float* k_sq_im, const float* rho_grad, const float* src,
                   int src_batch, int batch, int n_iter, float* res_hist, float* wf_hist, float* st_hist, float* rmse_hist, void* stream);

/* hn_fgmres_cycle_lossy with A_rho in its three places: the start residual, every w = A z, and the precond_iters iterations of hn_step_medium on
 * A z = precond_scale * v that make z_k (zero start, zero hidden states, z_k = wf / precond_scale, as hn_fgmres_cycle composes it).  precond_iters = 0
 * is plain restarted GMRES with zbasis == basis bit for bit.  Square domains only (HN_ERR_UNSUPPORTED on a rectangular one); not capturable; sums in a
 * fixed order.  rho_grad must be 16-byte aligned and overlap no other argument, as k_sq; so must k_sq_im where it is given. */
int hn_fgmres_cycle_medium(hn_ctx* ctx, float* x, const float* k_sq, const float* k_sq_im, const float* rho_grad, const float* rhs, int rhs_batch,
                           int batch, int restart, float tol, int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess,
                           float* rmse, int32_t* k_used, void* stream);

/* ---- absorbing media: the adjoint operator and adjoint-state gradients (added within ABI v7: new entry points, nothing existing changes) ----
 * With A u = L(u) + (k_sq + i k_sq_im) u the conjugate transpose is A^H g = L^H(g) + (k_sq - i k_sq_im) g:
 *     re = L^H(g)_re + k_sq g_re + k_sq_im g_im,   im = L^H(g)_im + k_sq g_im - k_sq_im g_re.
 * For A u = src, a real loss J, g = dJ/du (two real planes) and A^H lambda = g:
 *     dJ/dk_sq = -(lambda_re u_re + lambda_im u_im),   dJ/dk_sq_im = lambda_re u_im - lambda_im u_re,   dJ/dsrc = lambda.
 * Both line passes run on the LDS-line kernel the forward lossy operator runs on, at every size, the row pass with the conjugate pointwise term.
 *
 * hn_residual_vjp_lossy: out = A^H g; every legal square size and every rectangular domain.  Arguments as hn_residual_vjp, k_sq_im by k_sq's rules.
 * HN_ERR_ARG: a NULL pointer (a NULL k_sq_im with a message that names hn_residual_vjp), batch < 1, g == out, k_sq_im overlapping out.  On a square
 * domain that has tables to build, the first lossy call must not be under stream capture (HN_ERR_STATE, nothing enqueued), as for hn_residual_lossy. */
int hn_residual_vjp_lossy(hn_ctx* ctx, const float* g, const float* k_sq, const float* k_sq_im, float* out, int batch, void* stream);

/* hn_fgmres_adjoint_cycle on the lossy system A^H x = rhs: the start residual and every w = A^H z by the lossy adjoint; the preconditioner is
 * precond_iters iterations of hn_step_lossy between the same two similarity kernels and tables (a complex diagonal term commutes with W, so
 * A^T ~ W A W^-1 still holds); precond_iters == 0 is plain restarted GMRES on A^H with zbasis[:, j] == basis[:, j] bit for bit.  Square domains only
 * (HN_ERR_UNSUPPORTED on a rectangular one).  Workspaces, the capture refusal and every argument check are hn_fgmres_adjoint_cycle's; k_sq_im must be
 * 16-byte aligned and overlap no other argument, as k_sq. */
int hn_fgmres_adjoint_cycle_lossy(hn_ctx* ctx, float* x, const float* k_sq, const float* k_sq_im, const float* rhs, int rhs_batch, int batch, int restart,
                                  float tol, int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess, float* rmse,
                                  int32_t* k_used, void* stream);

/* hn_adjoint_grad with the third output g_k_sq_im [B,1,n,n] = lambda_re * u_im - lambda_im * u_re; one launch, no atomics.  g_k_sq and g_src are
 * hn_adjoint_grad's bit for bit.  g_k_sq_im is required, 16-byte aligned, and overlaps no other argument; every other rule is hn_adjoint_grad's
 * (HN_ERR_UNSUPPORTED on a rectangular domain).  A refused call leaves the outputs alone. */
int hn_adjoint_grad_lossy(hn_ctx* ctx, const float* lambda, const float* u, int src_batch, int batch, float* g_k_sq, float* g_k_sq_im, float* g_src,
                          void* stream);

/* ---- heterogeneous density: the adjoint operator and adjoint-state gradients (added within ABI v7: new entry points, nothing existing changes) ----
 * With D the Fourier first derivative of an axis and q = grad ln rho (real):
 *     A_rho u   = L(u) - b_x q_x D_x u - b_y q_y D_y u + (k_sq + i k_sq_im) u
 *     A_rho^H g = L^H g - D_x^H(conj(b_x) q_x g) - D_y^H(conj(b_y) q_y g) + (k_sq - i k_sq_im) g.
 * Per axis the lossy adjoint pass loads conj(a) g and conj(b) g; here the first of the two loads is conj(a - q b) g, q read from plane AXIS of rho_grad at
 * the element loaded.  Nothing else differs: no further buffer, no further transform; LDS and lines per block are the lossy adjoint pass's.
 * For A_rho u = src, a real loss J, g = dJ/du and A_rho^H lambda = g:
 *     dJ/dk_sq, dJ/dk_sq_im, dJ/dsrc    hn_adjoint_grad_lossy's formulas and bits
 *     dJ/dq_x = Re(conj(lambda) b_x D_x u),   dJ/dq_y = Re(conj(lambda) b_y D_y u)      (no dependence on q itself)
 *     dJ/dln rho = -(G_x dJ/dq_x + G_y dJ/dq_y),   dJ/drho = dJ/dln rho / rho
 * with G the real, antisymmetric map q = G ln rho of the axis (helmnet_amd.density.log_density_gradient; its transpose is -G, the Nyquist mode drops out).
 * The library computes dJ/dq; the last two lines belong to whoever made q (helmnet_amd.density.log_density_gradient_vjp for the spectral one).
 * The learned preconditioner of the adjoint cycle uses A^-H ~ conj(X A^-1 X^-1 conj(.)).  For the constant-density operators X = W = gamma_y[i] gamma_x[j];
 * here X = W / rho, because in the continuous problem A_rho = rho * (a W-symmetric operator).  Dense float64 A_rho of the ring medium (tests/
 * density_common.ring_medium), defect = ||A^T - X A X^-1||_F / ||A||_F, 2-norm = ||A^H M - I||_2 with M built from the exact inverse:
 *        n   max|q|   defect W   W/rho   W rho     2-norm W   W/rho   W rho
 *       32    0.21     0.056     0.034   0.107       2.40      0.19    5.75
 *       48    0.28     0.061     0.031   0.124       6.41      0.28   16.5
 * With W alone the exact inverse is not even a contraction; with W / rho it is.  So the cycle takes rho itself (only its ratios matter).
 * [measured, MI355X, profiles/density_bench.txt, third table] hn_residual_vjp_medium / hn_residual_vjp_lossy, alternating in one process: 1.113 at
 * 256^2 x 32, 1.133 at 512^2 x 16, 1.030 at 400^2 x 16; hn_adjoint_grad_medium 0.065 / 0.130 / 0.140 ms, about three quarters of one
 * hn_residual_vjp_medium (hn_adjoint_grad_lossy, a single pointwise launch: 0.011 / 0.015 / 0.011 ms).
 * [measured, profiles/adjoint_bench_density.txt] the adjoint solve to 1e-4, batch 4, restart 20, alpha 0.1 with density: plain 22 cycles / 0.034 s at
 * 96^2 and 26 / 0.062 s at 256^2; learned between W / rho 1 cycle (200 UNet evaluations) / 0.040 s and 1 / 0.049 s; learned between W alone (ones in
 * rho's place) the same within one inner step -- with the learned inverse the two weights cannot be told apart on this medium.
 *
 * hn_residual_vjp_medium: out = A_rho^H g; every legal square size and every rectangular domain.  Arguments as hn_residual_vjp_lossy, rho_grad
 * [B,2,h,w] behind k_sq_im, which MAY be NULL (a lossless medium).  HN_ERR_ARG: a NULL pointer (a NULL rho_grad with a message that names
 * hn_residual_vjp_lossy / hn_residual_vjp), batch < 1, g == out, k_sq_im or rho_grad overlapping out.  The tables and the capture rule are the lossy call's. */
int hn_residual_vjp_medium(hn_ctx* ctx, const float* g, const float* k_sq, const float* k_sq_im /* NULL: lossless */, const float* rho_grad,
                           float* out, int batch, void* stream);

/* hn_fgmres_adjoint_cycle_lossy on A_rho^H x = rhs.  rho: fp32 [B,1,n,n], > 0, read only, 16-byte aligned, overlapping nothing (as k_sq); it is read by
 * the preconditioner alone, normalised per sample by its first pixel rho[b,0,0,0] (a corner of the PML: the background), so that only ratios of rho
 * enter and the network sees the magnitude precond_scale sets, whatever the units of rho.  CALLER'S OBLIGATION: that pixel must hold the density
 * of the background medium (water in a skull map; helmnet_amd and the tests keep the PML in the background) -- a map whose corner is not the
 * reference density changes the magnitude the network sees, which costs cycles, not correctness (any positive weight leaves flexible GMRES exact): src = precond_scale * conj(v) * rho / W goes into precond_iters iterations of the hn_step_medium problem (zero start, zero
 * hidden states), and z = conj((W / rho) * wf) / precond_scale comes out (two streaming kernels, the lossy cycle's traffic plus the one plane; with
 * rho == 1 their bits are the lossy cycle's kernels').  precond_iters == 0 is plain restarted GMRES on A_rho^H: zbasis[:, j] == basis[:, j] bit for bit,
 * rho is not read and may be NULL.  precond_iters >= 1 with rho == NULL returns HN_ERR_ARG with a message that names rho.  Square domains only
 * (HN_ERR_UNSUPPORTED on a rectangular one); not capturable; every other rule is hn_fgmres_adjoint_cycle_lossy's, k_sq_im may be NULL. */
int hn_fgmres_adjoint_cycle_medium(hn_ctx* ctx, float* x, const float* k_sq, const float* k_sq_im /* NULL ok */, const float* rho_grad,
                           const float* rho /* [B,1,n,n], > 0; NULL allowed only with precond_iters == 0 */, const float* rhs, int rhs_batch, int batch,
                           int restart, float tol, int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess, float* rmse,
                           int* k_used, void* stream);

/* hn_adjoint_grad_lossy with one more output, g_rho_grad [B,2,n,n] = dJ/dq (plane 0: x, plane 1: y), per sample.  g_k_sq, g_k_sq_im and g_src are
 * hn_adjoint_grad_lossy's bit for bit (the same launch); with g_k_sq_im == NULL they are hn_adjoint_grad's.  g_rho_grad comes from two line passes
 * that transform u, multiply by i k alone, transform back and store Re(conj(lambda) b D u): one LDS buffer per line on a power-of-two size, two
 * otherwise.  g_rho_grad is required, 16-byte aligned, and overlaps no other argument.  Square domains only.  The line tables are the lossy route's: a
 * first call on a square domain that has them to build is refused under stream capture (HN_ERR_STATE, nothing enqueued); later calls are capturable. */
int hn_adjoint_grad_medium(hn_ctx* ctx, const float* lambda, const float* u, int src_batch, int batch, float* g_k_sq, float* g_k_sq_im /* NULL ok */,
                           float* g_rho_grad /* [B,2,n,n] */, float* g_src /* NULL ok */, void* stream);

/* ---- absorbing media in float64 (added within ABI v7: new entry points, nothing existing changes) ----
 * hn_residual_f64_lossy: res = L(wf) + (k_sq + i k_sq_im) wf - src in float64, hn_residual_f64's contract (res and / or rmse, the fixed-order
 * bit-reproducible sum, a first or growing call under stream capture HN_ERR_STATE with nothing enqueued, later calls capturable, wf may not overlap res,
 * 8-byte alignment) on every legal square size AND every rectangular domain, tensors [B,.,h,w].  It always runs the two float64 line passes (the FFT
 * route; there is no lossy dense kernel), whatever HN_OPT_F64_FFT says, and HN_CNT_F64_ROUTE reads 2 afterwards; on a square domain the dense route's
 * tables and bits are untouched and coexist with it.  On an h x w domain the column pass transforms w lines of length h with the y tables and the row
 * pass h lines of length w with the x tables; each pass has its own lines per block and LDS.  The lossy term is applied to the finished lossless value
 * (re -= k_sq_im * wf_im, im += k_sq_im * wf_re), so with k_sq_im == 0 res and rmse are bit for bit hn_residual_f64's on the FFT route (finite inputs).
 * k_sq_im: [B,1,h,w] double, read only; NULL returns HN_ERR_ARG with a message that names hn_residual_f64; overlapping res returns HN_ERR_ARG.  What
 * the first call builds is freed by hn_set_domain / hn_set_domain_rect / hn_destroy.
 * [measured, MI355X, profiles/f64_lossy_bench.txt] lossy / lossless time on the FFT route (res + rmse, alternating in one process): 1.009 at
 * 256^2 x 32 (0.106 ms), 1.013 at 512^2 x 16 (0.258 ms), 1.029 at 2048^2 x 1 (0.470 ms): the one more plane read; 256 x 1024 x 8: 0.130 ms. */
int hn_residual_f64_lossy(hn_ctx* ctx, const double* wf, const double* k_sq, const double* k_sq_im, const double* src, int src_batch,
                          double* res, double* rmse, int batch, void* stream);

/* hn_fgmres_refine_cycle with the lossy operator in all three places: the float64 residual (hn_residual_f64_lossy's, k_sq_im up-cast exactly beside
 * k_sq), the fp32 cycle (hn_fgmres_cycle_lossy's launches) and the preconditioner (hn_step_lossy); precond_iters == 0 is plain refined GMRES.  rmse64
 * is bit for bit hn_residual_f64_lossy's; basis, zbasis, hess, rmse and k_used are bit for bit hn_fgmres_cycle_lossy's on the scaled right-hand side
 * from x = 0.  Square domains only (HN_ERR_UNSUPPORTED on a rectangular one).  Every other refusal, the workspaces and "not capturable" are
 * hn_fgmres_refine_cycle's; k_sq_im must be 16-byte aligned and overlap no other argument, as k_sq; NULL returns HN_ERR_ARG with a message that names
 * hn_fgmres_refine_cycle. */
int hn_fgmres_refine_cycle_lossy(hn_ctx* ctx, double* x, const float* k_sq, const float* k_sq_im, const float* rhs, int rhs_batch, int batch, int restart,
                                 double tol, float inner_floor, int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess,
                                 float* rmse, int32_t* k_used, double* rmse64, void* stream);

/* ---- training step (hybridnet.py:385-413 training_step, :250-283 configure_optimizers, :172-176
 * on_after_backward).  The caller owns every training tensor: the weights as ONE flat device blob in the order of
 * hn_load_weights (PyTorch layouts inside: conv [out,in,kh,kw], transposed conv [in,out,kh,kw]), its gradient, and the
 * Adam moments -- so a data-parallel job all-reduces `grad` as a single 193 KB bucket (RCCL) between the two calls and a
 * checkpoint is those tensors.  The context supplies the architecture (depth / activation of the last hn_load_weights),
 * the spectral tables of hn_set_domain and the activation tape (grown on demand; hn_train_reserve pre-allocates).
 * fp32 throughout; gradients are accumulated in a fixed order (per-block partial sums + one reduction, no atomics):
 * bit-reproducible.  Levels without state (state_depth < depth) are handled by the caller's packing: zero-padded weights whose entries
 * it marks non-trainable in hn_adam_step. */

/* Pre-allocate the tape for `batch` samples x `n_unroll` unrolled iterations (optional). */
int hn_train_reserve(hn_ctx* ctx, int batch, int n_unroll);

/* Loss and gradients of n_unroll unrolled solver iterations started from (wf, res, states):
 *     for t < n_unroll: d = HybridNet_w(cat[wf, 1e3*res, sigmas]); wf += d/1e3; res = L(wf) + k_sq*wf - src   (single_step :558-584)
 *     loss = loss_scale * mean over (n_unroll, B, 2, n, n) of res_t^2        (training_step :403-409, loss_scale = 1e4)
 * Inputs (device, not modified): weights [hn_weight_count], wf / res [B,2,n,n], states [B,2,L], k_sq [B,1,n,n],
 * src [src_batch,2,n,n].  Outputs (device): wf_hist / res_hist [n_unroll,B,2,n,n] and st_hist [n_unroll,B,2,L] (required: the
 * lists n_steps(..., True, True) returns, :586-623 -- they are also the tape of the backward pass); loss [1];
 * grad [hn_weight_count] = d loss / d weights (overwritten); grad_wf0 / grad_res0 [B,2,n,n], grad_st0 [B,2,L] =
 * d loss / d (wf, res, states) (optional, NULL to skip).
 * Stream capture (a caller recording the step into a HIP graph): supported with the workspace in place -- call hn_train_reserve (or run
 * one eager hn_train_grad of the same shape) first; a captured call whose workspace would have to grow returns HN_ERR_STATE instead of
 * breaking the capture.  The launch tables of a captured call live in a pinned buffer of their own that eager calls never rewrite; capturing a
 * SECOND graph on the same context rewrites it (one captured training step per context at a time).  Once a call has been captured, an eager call that
 * needs a LARGER workspace (bigger batch, more unrolled iterations, another domain) returns HN_ERR_STATE instead of freeing memory the graph points into:
 * destroy the graph and call hn_train_reserve (the caller's word that no captured step is replayed any more; it may re-allocate). */
int hn_train_grad(hn_ctx* ctx, const float* weights, const float* wf, const float* res, const float* states, const float* k_sq,
                  const float* src, int src_batch, int batch, int n_unroll, float loss_scale, float* wf_hist, float* res_hist,
                  float* st_hist, float* loss, float* grad, float* grad_wf0, float* grad_res0, float* grad_st0, void* stream);

/* ---- reverse mode of the solver loop (added within ABI v7: a new entry point, nothing existing changes, so HN_ABI_VERSION stays 7) ----
 * hn_step_vjp: the vector-Jacobian product of n_iter iterations of hn_step (single_step, hybridnet.py:558-584, looped as in forward :654-697),
 * i.e. what torch.autograd computes when the reference back-propagates through its solver.  Iteration t maps (wf, res, st)_{t-1} -> (wf, res, st)_t,
 * where index -1 is (wf0, res0, states0) and index t is slot t of the histories hn_step wrote (all three required: they are the tape, the
 * linearisation point of every iteration).  The UNet activations of each iteration are recomputed in reverse order by the training forward pass
 * (hn_train_grad's kernels), so the workspace holds the activations of TWO iterations whatever n_iter is.
 * Cotangents (device, NULL = zero): g_wf_hist / g_res_hist [n_iter,B,2,n,n] and g_st_hist [n_iter,B,2,L] on the histories; g_wf_T / g_res_T /
 * g_st_T [B,...] on the last iteration's outputs (added to slot n_iter - 1: a caller that only uses the end passes no histories).
 * Outputs: g_wf0 / g_res0 [B,2,n,n], g_st0 [B,2,L] OVERWRITTEN (NULL = skip); g_k_sq [B,1,n,n], g_src [src_batch,2,n,n] and g_weights
 * [hn_weight_count] ACCUMULATED (+=; NULL = skip -- without g_weights no weight-gradient kernel runs).  The source map itself is not read
 * (the residual is linear in it), only its batch: src_batch 1 (broadcast: the gradient is summed over the batch once, at the end, in sample
 * order) or B.  weights: the blob in PyTorch layout, as hn_train_grad takes it.  Levels without state (zero-padded weights, see hn_train_grad)
 * get a zero state gradient out of the kernels: their slots pass through the solver unchanged, so their cotangent is the caller's identity.
 * flags (a caller that splits a long solve into segments -- re-running each with hn_step from a checkpoint -- and wants the bits of ONE call):
 *   HN_VJP_DEFER    keep the weight / broadcast-source partial sums in the context's workspace instead of reducing them into g_weights / g_src;
 *   HN_VJP_CONTINUE add to the partial sums the previous call left (it must have been an hn_step_vjp with HN_VJP_DEFER of the same batch and
 *                   domain, with no other training call on the context in between and no re-allocation of its workspace; HN_ERR_STATE otherwise --
 *                   the tape has two slots whatever n_iter is, so the segments of one sweep never re-allocate it).
 *   Segments processed last to first with DEFER on all but the first segment and CONTINUE on all but the last segment give the gradients of one call
 *   bit for bit.  The input gradients and g_k_sq need no flag: a segment's g_wf0 / g_res0 / g_st0 is the earlier segment's g_*_T.
 * fp32 UNet arithmetic only (HN_PREC_FP32 / HN_PREC_FP32_VALU; HN_ERR_UNSUPPORTED in the 16-bit modes).  Bit-reproducible: fixed-order sums, no
 * atomics.  The weight-gradient launches run beside the chain as HN_OPT_TRAIN_OVERLAP says, handed over with events (not the device words of
 * HN_OPT_SIDE_SYNC); HN_EXP_TRAIN_LANES does not apply (one chain).  NOT capturable: under stream capture it returns HN_ERR_STATE before
 * enqueuing anything (it may grow its workspace and paces its pinned job tables on the host). */
enum hn_vjp_flags { HN_VJP_CONTINUE = 1, HN_VJP_DEFER = 2 };
int hn_step_vjp(hn_ctx* ctx, const float* weights, const float* wf0, const float* res0, const float* states0, const float* k_sq, int src_batch,
                int batch, int n_iter, const float* wf_hist, const float* res_hist, const float* st_hist, const float* g_wf_hist,
                const float* g_res_hist, const float* g_st_hist, const float* g_wf_T, const float* g_res_T, const float* g_st_T, float* g_wf0,
                float* g_res0, float* g_st0, float* g_k_sq, float* g_src, float* g_weights, int flags, void* stream);

/* ---- forward mode of the solver loop (added within ABI v7: a new entry point, nothing existing changes, so HN_ABI_VERSION stays 7) ----
 * hn_step_jvp: the Jacobian-vector product of n_iter iterations of hn_step, i.e. what torch.autograd.forward_ad computes when a dual tensor runs
 * through the reference's solver.  Iteration t maps (wf, res, st)_{t-1} -> (wf, res, st)_t as in hn_step_vjp: index -1 is (wf0, res0, states0) and
 * index t is slot t of the histories hn_step wrote from them (all three required: they are the tape, the linearisation point of every iteration).
 * The UNet's primal activations are recomputed from the slot in front of each iteration beside the tangents (packed duals: a float2 (primal,
 * tangent) per activation, one packed FMA per tap, hn_jvp.hip) and discarded: only tangents leave an iteration, memory does not grow with n_iter.
 *     d' = J_net [wf', 1e3 res', 0, 0; st'];  wf' = d' / 1e3 + wf';  res' = L(wf') + k_sq * wf' + k_sq' * wf_t - src'
 * In / out (device, in place): t_wf / t_res [B,2,n,n], t_states [B,2,L]: the tangents of (wf0, res0, states0) on entry, of the last iteration's
 * outputs on return.  In (NULL = zero): t_k_sq [B,1,n,n], t_src [src_batch,2,n,n], the same direction at every iteration.  Out (optional, NULL =
 * skip): t_wf_hist / t_res_hist [n_iter,B,2,n,n], t_st_hist [n_iter,B,2,L], the tangents after every iteration.  The source map itself is not read,
 * only its batch (1 or B).
 * It linearises the network of the last hn_load_weights; there are NO weight tangents (the weights are constants of the linearisation).  fp32 UNet
 * arithmetic only (HN_ERR_UNSUPPORTED in the 16-bit modes, as hn_step_vjp).  Levels without state (zero-padded weights, see hn_train_grad) get a
 * zero state tangent out of the kernels: their slots pass through the solver unchanged, so their tangent is the caller's identity.
 * Alignment: any 4-byte-aligned pointers, like hn_step (the dual kernels use scalar accesses to the caller's tensors).
 * Overlap: t_wf, t_res, t_states and the three tangent histories are written; a written tensor may overlap no other tensor of the call, tensors that
 * are only read may share memory.  An overlap returns HN_ERR_ARG "hn_step_jvp: <a> overlaps <b>" with nothing enqueued.
 * Other refusals: HN_ERR_ARG for a NULL required pointer, n_iter < 1, batch < 1, src_batch not in {1, batch}; HN_ERR_STATE before hn_load_weights or
 * hn_set_domain.
 * Workspace: the dual activations, a second tangent-state buffer and the tangent source s~ = src' - k_sq' * wf_t, built by the first call and grown
 * by a larger batch; hn_load_weights, hn_set_domain and hn_destroy free it.  Such a first or growing call under stream capture returns HN_ERR_STATE
 * before enqueuing anything; later calls are plain launches on the caller's stream (no side stream, no device words, no atomics) and can be captured.
 * Determinism: two calls on equal inputs give equal bits; a sample's tangents do not depend on its batch mates; n_iter = a + b in one call equals two
 * calls of a and b bit for bit (the second fed the first's t_* and the tape's slot a - 1 as its (wf0, res0, states0)); t_res of every iteration
 * equals, bit for bit, hn_residual(t_wf, k_sq, s~) with s~ composed by the caller (one rounded product, one rounded difference). */
int hn_step_jvp(hn_ctx* ctx, const float* wf0, const float* res0, const float* states0, const float* k_sq, int src_batch, int batch, int n_iter,
                const float* wf_hist, const float* res_hist, const float* st_hist, float* t_wf, float* t_res, float* t_states, const float* t_k_sq,
                const float* t_src, float* t_wf_hist, float* t_res_hist, float* t_st_hist, void* stream);

/* ABI v5.  `event` (a hipEvent_t, or NULL to clear): every later hn_train_grad on this context records it on the caller's stream BEHIND THE FORWARD SWEEP, i.e. when
 * wf_hist / res_hist / st_hist are complete and before the backward pass starts.  The reference's training_step decides from the residual of one
 * unrolled iteration which replay-buffer slots to refill (`res.pow(2).mean() < 1`, hybridnet.py:431-463) -- a host decision; with this event the host
 * takes it while the backward pass runs instead of draining the queue after it (helmnet_amd.training.Trainer).
 * `sumsq_host` (optional; pinned host memory of `sumsq_capacity` floats): the forward sweep's own table of sum over (2, N, N) of res^2, one float per
 * (iteration t, sample b) at [t * batch + b], is copied there before the event is recorded -- the refill rule needs nothing else, so no kernel of the
 * caller has to run between the two sweeps.  The sums are accumulated with float atomics (their last bits are not reproducible, like `loss`).
 * hn_train_grad returns HN_ERR_ARG if n_unroll * batch exceeds the capacity.  The caller owns event and table; not recorded / copied by a call that is
 * being captured into a HIP graph. */
int hn_train_set_forward_event(hn_ctx* ctx, void* event, float* sumsq_host, int64_t sumsq_capacity);

/* ABI v5.  Rows of the caller's replay buffer (replaybuffer.py:20-47; hybridnet.py:388-397 sample, :436-463 refill).  The reference keeps a Python list of
 * `capacity` Experience tuples; on the device that is one [capacity, row_floats[f]] fp32 array per field f (wavefield, hidden state, k_sq, residual,
 * source: n_fields <= 8), owned by the caller.  `slots`: `count` HOST integers in [0, capacity) -- they travel in the kernel arguments, so neither
 * call copies anything to the device or waits for it.
 *   hn_rows_gather : out[f][j, :] = buffers[f][slots[j], :]            (ReplayBuffer.sample's `stack`, all fields in one launch)
 *   hn_rows_scatter: buffers[f][slots[j], :] = rows[f][j, :]           (ReplayBuffer.append for a batch of slots); rows[f] == NULL writes zeros (the
 *                    wavefield and hidden state of a fresh experience, :456-458); rows_stride[f] = floats between consecutive new rows, 0 = the same row for
 *                    every slot (the one source map, :462); rows_stride == NULL means row_floats.  Slots must be distinct (as `sample` draws them).
 * HN_ERR_ARG for a slot outside the buffer, a NULL array, more than 8 fields. */
int hn_rows_gather(hn_ctx* ctx, int n_fields, const float* const* buffers, const int64_t* row_floats, int64_t capacity, const int32_t* slots,
                   int count, float* const* out, void* stream);
int hn_rows_scatter(hn_ctx* ctx, int n_fields, float* const* buffers, const int64_t* row_floats, int64_t capacity, const int32_t* slots, int count,
                    const float* const* rows, const int64_t* rows_stride, void* stream);

/* ---- a stream of maps solved to a tolerance (added within ABI v7: new entry points, nothing existing changes) ----
 * The reference's evaluate.py runs a test set batch by batch for a fixed iteration count; a batch solved to a tolerance instead stops with its
 * WORST map.  These two calls are what a scheduler needs to stop every map on its own and hand its slot of the batch to the next map
 * (helmnet_amd.IterativeSolver.solve_many): the batch arrays wf / res [batch,2,n,n], states [batch,2,L], k_sq [batch,1,n,n] (and src
 * [batch,2,n,n] when every map has its own source) are SLOTS, the maps of the job live in sos_in [n_maps,1,n,n] (and src_in [n_maps,2,n,n]).
 * Both work in every hn_precision mode (no UNet arithmetic) and are NOT capturable: they read host lists / hand out a host table, and return
 * HN_ERR_STATE under stream capture before enqueuing anything.
 *
 * hn_stream_verdict: one launch that reads the rmse_hist rows [n_rows, batch] a chunk of hn_step iterations wrote and leaves one record per slot
 * in a pinned, host-mapped table of the context (sized by hn_reserve, grown on demand): first_below = first row whose RMSE is < tol (-1: none),
 * last_rmse = the last row's RMSE, bad = 1 if any row is NaN / Inf or > diverge_rmse (pass +Inf for "never").  One thread walks one slot's column
 * in row order: deterministic, no atomics.  *host_table is valid once `stream` has been synchronised and until the next call on this context.
 *
 * hn_stream_swap: retire and refill, one launch per 192 operations (the list travels in the kernel arguments like the slots of hn_rows_gather; a
 * longer list is split).  ops: `count` HOST records; per record, in this order (-1 = none):
 *   retire_map  out_wf[retire_map] = wf[slot], and out_res[retire_map] = res[slot] if out_res is not NULL;
 *   move_from   the wf, res, states, k_sq (and, with src_batch == batch, src) rows of slot move_from are copied into slot (tail compaction);
 *   refill_map  the slot becomes what IterativeSolver.forward starts from for map refill_map: k_sq = ((1 / sos) * omega)^2 in fp32 (the
 *               arithmetic of get_initials, hybridnet.py:522-538), wf = 0, states = 0, res = k_sq * 0 - src (with src_batch == batch the slot's
 *               src row is src_in[refill_map] first; else src is the one broadcast map) -- no spectral launch: L(0) = 0.
 * HN_ERR_ARG for: a slot outside [0, batch) or a map outside [0, n_maps); a slot named by two records; two records retiring the same map; a
 * move_from that is the record's own slot or a slot another record of the call moves into / refills; src_batch not in {1, batch}; a refill without
 * sos_in, or without src_in when src_batch == batch (with batch == 1 a NULL src_in means the broadcast source); a retire without out_wf; rows or pointers that are not 16-byte multiples. */
typedef struct hn_stream_verdict_rec { int32_t first_below; int32_t bad; float last_rmse; } hn_stream_verdict_rec;
typedef struct hn_stream_op { int32_t slot, retire_map, move_from, refill_map; } hn_stream_op;
int hn_stream_verdict(hn_ctx* ctx, const float* rmse_hist, int n_rows, int batch, float tol, float diverge_rmse,
                      const hn_stream_verdict_rec** host_table, void* stream);
int hn_stream_swap(hn_ctx* ctx, float* wf, float* res, float* states, float* k_sq, float* src, int src_batch, int batch,
                   int count, const hn_stream_op* ops, const float* sos_in, const float* src_in, int64_t n_maps, float omega,
                   float* out_wf, float* out_res, void* stream);

/* One optimiser step on caller-owned device arrays of n floats: gradient value clipping to [-clip_value, clip_value]
 * (clip_value <= 0: none; torch.nn.utils.clip_grad_value_, hybridnet.py:172-176), then torch.optim.Adam as configured by the
 * reference (hybridnet.py:250-258: betas (0.9, 0.95), L2 weight decay added to the gradient, no amsgrad):
 *     g += weight_decay * p;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps)
 * `step` counts from 1.  `trainable` (n bytes on the device): entries with 0 are left untouched.  It may be NULL only for a PReLU network
 * with state at every level: for the parameter-free activations the blob's slope slots hold CONSTANTS (leakyrelu 0.01 ...) with zero
 * gradient, which weight decay + Adam's normalisation would move by about lr per step, and the zero padding of a level without state
 * (state_depth < depth) likewise -- helmnet_amd.training.trainable_mask builds the mask.  A NaN gradient entry stays NaN through the
 * clipping (as torch's clamp_) and makes that weight NaN: a diverged step is visible, not silently applied. */
int hn_adam_step(hn_ctx* ctx, float* weights, const float* grad, float* exp_avg, float* exp_avg_sq, const unsigned char* trainable,
                 size_t n, float lr, float beta1, float beta2, float eps, float weight_decay, float clip_value, int64_t step,
                 void* stream);

/* Test / debugging aid: copy one tensor of the LAST unrolled iteration processed by hn_train_grad's backward sweep (i.e.
 * iteration 0 of the call) out of the library's workspace into `out` (device, at most max_floats; returns the number of floats
 * the tensor has, or a negative hn_status).  kind: 0 x_d (level input), 1 conv_signal mid, 2 out_d (skip), 3 conv_state mid,
 * 4 upsampled u_d, 5 decoder mid (level == depth: bottleneck), 6 decoder output y_d, 7 inc mid; 16 + k: the gradient of the
 * loss with respect to tensor kind k in {0, 2, 4, 6}. */
int64_t hn_train_peek(hn_ctx* ctx, int kind, int level, float* out, int64_t max_floats, void* stream);

/* Optional per-kernel timing (measurement only; bench.py's roofline block uses it).  While a
 * kernel id's bit is set in `kernel_mask`, every launch of that kernel inside hn_step / hn_unet /
 * hn_residual is bracketed by a HIP event pair recorded on the caller's stream.  Kernel ids:
 *   0 inc | 1+3d conv_signal(d) | 2+3d conv_state(d) | 3+3d down(d) | 19 bottleneck |
 *   20+2d up(d) | 21+2d decoder(d) (d=0 includes outc + wavefield update) |
 *   32 spectral column pass | 33 spectral row pass (or the dense operator) |
 *   34 the fused deepest level (conv_signal, conv_state, down, bottleneck, up, decoder of level depth-1 in one kernel;
 *      those six ids then do not occur) | 35 both spectral passes under ONE event pair
 *      | 36 inc and conv_signal_0 as one launch (HN_OPT_DC_PAIR; ids 0 and 1 then do not occur).
 * hn_profile_collect synchronises the recorded events, returns per-id total milliseconds and
 * launch counts for ids [0, n_ids) and resets the accumulators. */
#define HN_KERNEL_IDS 37
int hn_profile_enable(hn_ctx* ctx, uint64_t kernel_mask);
/* Bracket only every `every_nth` launch of a selected kernel (default 1), starting every_nth / 2 launches in.  An event pair
 * costs a few microseconds of stream gap, so timed runs sample instead of bracketing every launch. */
int hn_profile_stride(hn_ctx* ctx, int every_nth);
int hn_profile_collect(hn_ctx* ctx, double* total_ms, int64_t* count, int n_ids);
/* Shortest bracketed launch per kernel id in the interval closed by the last hn_profile_collect
 * (robust against host-side launch stalls, which inflate event-bracketed times). */
int hn_profile_min(hn_ctx* ctx, double* min_ms, int n_ids);

#ifdef __cplusplus
}
#endif
#endif /* HELMNET_HIP_H */
