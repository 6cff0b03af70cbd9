/*
 * p2phd.h -- C ABI of libp2phd_hip.so: the MI355X (gfx950) hot path of pix2pixHD audio
 * super-resolution (batched MDCT4/IMDCT4 + generator/discriminator conv stack).
 *
 * The reference (ishine/pix2pixHDAudioSR) has no FFI on this path: its boundary is the Python
 * module API (models/mdct.py, models/networks.py, models/pix2pixHD_model.py).  Every entry
 * point below names the reference code it replaces (file:line relative to the reference
 * checkout); the Python mirror of those modules in pix2pixhdaudiosr_amd/ binds these symbols
 * with ctypes (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - all data pointers are DEVICE pointers, caller-allocated (torch tensors own them);
 *   - `stream` is a hipStream_t passed as void* (the caller's current stream); no entry point
 *     allocates, frees or synchronises, so calls are graph-capturable;
 *   - return 0 on success, a negative P2PHD_E* code otherwise; p2phd_last_error() gives text
 *     (thread-local);
 *   - thread-compatible, not thread-safe per output buffer.
 *
 * Streams
 *   The kernels that reduce across workgroups without float atomics (InstanceNorm backward sums, bias column sums, loss
 *   accumulators, the split-K tail of the conv GEMM) keep their partial rows and arrival tickets in a scratch that belongs
 *   to the library, one region per kernel family.  A region serves ONE stream at a time: every such launch records an event
 *   behind itself, and a call of the same family that arrives on another stream first makes that stream wait for the event
 *   (hipStreamWaitEvent) -- the launches are ordered on the device, no partials mix, nothing is refused and no stream handle
 *   is ever queried after its owner may have destroyed it.  Launches recorded into a graph under capture run in graph order;
 *   replaying two graphs that use one family concurrently on two streams is the caller's to order.  p2phd_reduction_reset(stream)
 *   re-arms the tickets; call it once per training step (a faulted or aborted launch could otherwise leave one armed wrong).
 */
#ifndef P2PHD_H
#define P2PHD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2PHD_OK            0
#define P2PHD_EINVAL       -1   /* bad argument / unsupported geometry */
#define P2PHD_ELAUNCH      -2   /* HIP launch error */
#define P2PHD_EUNSUPPORTED -3   /* valid request this build does not implement */

/* element types of activation / weight buffers.  P2PHD_BF16 names THE LIBRARY'S 16-BIT STORAGE TYPE: bf16 in libp2phd_hip.so
 * (the benchmarked mode), IEEE fp16 in libp2phd_hip_f16.so -- the same sources built with -DP2PHD_F16 (the reference's actual AMP
 * type: train.py:62-67 runs torch.cuda.amp.autocast, i.e. fp16 activations with fp32 accumulation and a GradScaler).  Same entry
 * points, same layouts; p2phd_half_type() returns 1 (bf16) or 2 (fp16). */
#define P2PHD_F32  0
#define P2PHD_BF16 1
int p2phd_half_type(void);

const char* p2phd_last_error(void);
int p2phd_abi_version(void);
/* fills name (<= cap bytes) with the device's gcnArchName; returns CU count or <0 */
int p2phd_device_info(char* name, int cap);
/* Per-library options (process-wide; tests, A/B timing, and one that the data-parallel step sets).  Unknown name or value: P2PHD_EINVAL.
 *   "cus" n            CUs a conv launch may count on when the step runs on a CU-masked stream (0 = all of the device's)
 *   "gconv_bm" v       gather-GEMM tile: 0 heuristic | 128 | 192 | 256 | 258 (256 rows on the 2-slot ring) | 512 (256 x 256)
 *   "gconv_halo" 0|1   the HALO main loop of 3x3 stride-1 layers on 16-wide planes (1) or the generic loop (0)
 *   "tile128x192" 0|1  the 128 x 192 tile of small planes with 192-divisible outputs
 *   "cls_skip" 0|1     tap-skipping merged stride-2 launches (changes the packed layout of those layers: see p2phd_conv_pack_layout)
 *   "splitk_tail" 0|1|2  split-K of the last, partly filled tile round: off | where the cost model says so | wherever possible
 *   "march", "dfirst", "dlast", "c7_generic", "reflect_generic", "mdct_generic" 0|1   the dedicated kernels of the outermost
 *                      stride-2 pair, the discriminator's first / last layer, the two 7x7 layers, the reflection extras, the fast MDCT:
 *                      on (default; c7_generic / reflect_generic / mdct_generic = 1 select the generic path instead)
 *   "wgrad_tm" 0|128, "wgrad_xcd" 0|1, "mdct_iters" 0..8, "c7_abl"   weight-gradient row tile / XCD-aware order, experiment knobs
 *   "truepeak_grid" n  workgroups per row of p2phd_truepeak at most (0 = one per tile, as far as the partial table has rows; 1 .. 65536:
 *                      tests run the path on which a workgroup walks several tiles at a small size); the result's bits do not depend on it
 *   "limiter_grid" n   workgroups of p2phd_limiter_envelope and of p2phd_limiter_apply at most (0 = one per tile, as far as the partial table
 *                      has rows; 1 .. 16384: tests run the path on which a workgroup walks several tiles); the result's bits do not depend on it
 *   "speechlevel_grid" n  workgroups per row of p2phd_speechlevel_envelope and of p2phd_speechlevel_counts at most (0 = one per tile up to
 *                      2048; 1 .. 16384: tests run the path on which a workgroup walks several tiles); the result's bits do not depend on it
 *   "cw_inject" 0|1    libp2phd_hip_chk.so only: selects round 4's too-lax HALO wait (sensitivity check of p2phd_wait_check) */
int p2phd_set_option(const char* name, int value);
/* zeroes the arrival tickets of the fixed-order reductions on `stream` (17 KB memset; see "Streams" above) */
int p2phd_reduction_reset(void* stream);
/* Measurement hook (bench.py's roofline): while armed, every launch of the implicit-GEMM conv kernel whose gathered
 * tensor has `cin_pitch` channels, whose GEMM-K is `kk` and whose pixel grid is hg x wg is bracketed by HIP events on its
 * own launch stream (the kernel alone: none of the companion launches of p2phd_conv_fwd).  p2phd_probe_read waits for
 * the recorded events and returns up to `cap` durations in milliseconds; arm with enable = 0 to stop. */
int p2phd_probe_gconv(int enable, int cin_pitch, int kk, int hg, int wg);
/* Same with two more filters: gather_pad_mode = the padding rule of the launch's gather (0 zeros, 1 reflect = the forward of
 * a ReflectionPad2d conv, 2 = the reflect adjoint of its input gradient; -1 = any) and elem_bytes = operand element size
 * (1 e4m3, 2 bf16, 4 f32; 0 = any) -- so a forward launch is told from the same-shaped input-gradient launch. */
int p2phd_probe_gconv_ex(int enable, int cin_pitch, int kk, int hg, int wg, int gather_pad_mode, int elem_bytes);
int p2phd_probe_read(float* ms_out, int cap);
/* Launch counters: how many launches of a kernel family the library has made since the last reset -- "gconv" (every
 * gather-GEMM launch), "halo" (those on the patch-staged 3x3 main loop), "cls_skip" (tap-skipping merged stride-2 launches),
 * "splitk" (launches with a split-K tail), "tile256" (256 x 256 tiles), "tile128x192" (128 x 192 tiles of small planes),
 * "march" / "march_w" (marching kernels), "wgrad" (MFMA weight gradient), and the dedicated single-layer kernels "dfirst",
 * "dlast", "c7" (the 7x7 end layers) and "thin_wgrad" (calls routed to them), "timed_pack" / "timed_frames" (the time-domain
 * discriminator's pair pack and spectrogram <-> frames kernels, csrc/timed.hip), "stitch" (the segment gather and the
 * cross-fading stitch of whole-file generation, csrc/stitch.hip), "pcm" (the PCM decode, encode, peak report and extended encode of its file
 * ends, csrc/pcm.hip), "metrics_rows" (the per-row metrics, csrc/metrics.hip), "xover" (the time-domain crossover of whole-file
 * generation, csrc/xover.hip), "specimg" (the STFT and the renderer of its spectrogram picture, csrc/specimg.hip), "loudness" (the
 * BS.1770 hop energies, the gate and the loudness range of whole-file generation, csrc/loudness.hip), "truepeak" (the oversampling true-peak measurement
 * of whole-file generation, csrc/truepeak.hip), "limiter" (the envelope and the gain curve of its look-ahead true-peak limiter,
 * csrc/limiter.hip), "bandwidth" (the long-term average spectrum and the band-edge decision of its bandwidth report,
 * csrc/bandwidth.hip), "stereo" (the cross-spectrum and the band sums of its stereo image report and the mid/side matrix of
 * stereo='ms', csrc/stereo.hip), "rateconv" (the rate converter of its output stage, csrc/rateconv.hip), "normscope" (the range
 * pre-pass and the encode under a given range of its norm_scope='clip', csrc/spectro.hip: one per call that launches anything),
 * "shaper" (the noise-shaped dither of its PCM16 encoder, csrc/shaper.hip), "flac" (the two kernels of its FLAC input,
 * csrc/flac.hip: a p2phd_flac_decode with nframes > 0 counts 2), "flacenc" (the three kernels of its FLAC output, csrc/flacenc.hip:
 * a p2phd_flac_encode counts 3), "wavcodec" (the G.711 and IMA ADPCM decoders of its coded WAV input, csrc/wavcodec.hip: one per
 * call with frames > 0), "speechlevel" (the envelope, the counts and the decision of its active speech level, csrc/speechlevel.hip:
 * one per entry with frames > 0), "normrows" (the per-row statistics, encode and decodes of its segment_norm, csrc/spectro.hip: one
 * per call that launches anything), and the weight packs of p2phd_conv_pack_weights /
 * p2phd_conv_fp8_pack_weights, one family per kernel of csrc/wpack.hip, counted per launch plan: "wpack_generic" (the tap walk),
 * "wpack_dense", "wpack_transposed" (the two LDS re-orderings), "wpack_kmajor" (cast of K-major master weights), "wpack_kmajor_t"
 * (their per-tap transpose), "wpack_merged" (merged sub-pixel launches, either tap order), "wpack_fp8" (the e4m3 quantiser with
 * its amax and scale kernels), and "wpack_frag" (the fragment pack of a dedicated kernel behind the generic pack).
 * family == NULL with reset != 0 clears all.
 * Returns the count before the reset, -1 for an unknown name.  Counts launches recorded under graph capture once (at capture).
 * Test hook: proves which kernels a whole training step really runs on (train.py:148-184 at the benchmarked batch). */
int64_t p2phd_launch_count(const char* family, int reset);
/* Checker of the hand-counted LDS-DMA waits (round 5; libp2phd_hip_chk.so = the same sources with -DP2PHD_CHECK_WAITS): every
 * wave of the gather-GEMM loops (generic and HALO) and of the weight-gradient loops logs the LDS buffer each piece it issues
 * fills and, at every relaxed `s_waitcnt vmcnt(n)` in front of a slab barrier, checks that none of its n youngest pieces targets
 * a buffer that is read behind that barrier.  out4[0] = violating kernel families (bit 0 generic loop, 1 HALO, 2 weight gradient,
 * 3 its f32 form), [1] = waits checked, [2] = first offender, [3] = pieces logged.  Synchronises the device.  The product
 * build returns P2PHD_EUNSUPPORTED.  p2phd_set_option("cw_inject", 1) (check build only) runs the HALO loop with the too-lax
 * wait that shipped for 1.5 h in round 4: the checker must flag it (tests/test_gpu_waits.py). */
int p2phd_wait_check(unsigned* out4, int reset);

/* ------------------------------------------------------------------------------------------
 * MDCT4 / IMDCT4 (models/mdct.py:461-566).  n_fft a power of two in [16, 4096].
 *
 * Tables: p2phd_mdct4_tables_floats(n_fft) floats, filled on the HOST by
 * p2phd_mdct4_tables_fill (fp64 trigonometry rounded once to fp32), uploaded by the caller and
 * passed back as the device pointer `tables`.  They replace exp1/exp2 of mdct.py:483-484,539-540.
 * ---------------------------------------------------------------------------------------- */
size_t p2phd_mdct4_tables_floats(int n_fft);
int p2phd_mdct4_tables_fill(int n_fft, float* host_out);

/* Frame geometry exactly as MDCT4.forward computes it (mdct.py:488-500), including the
 * len(signal) quirk: dim0 is the size of the first dimension of the input (the batch size for a
 * [B,T] signal, T for a 1-D one).  Pure host integer arithmetic. */
int p2phd_mdct4_frame_layout(int64_t dim0, int64_t T, int hop, int win, int center,
                             int64_t* start_pad, int64_t* end_pad, int64_t* n_frames);

/* Framed transform: out[b,t,k] = scale * sum_n w[n] xpad[b, t*hop+n] cos(2pi/N (n+1/2+N/4)(k+1/2)),
 * xpad = x shifted right by start_pad with zeros outside [0,T).  x [B,T] f32, window [win] f32,
 * out [B,F,N/2] f32.  MDCT4.forward (mdct.py:486-513) = this with scale 1; the backward of
 * IMDCT4 = this with x = grad, start_pad = crop, scale 4/N. */
int p2phd_mdct4_fwd(const float* x, int64_t B, int64_t T, int n_fft, int hop, int win,
                    const float* window, const float* tables, int64_t start_pad, int64_t n_frames,
                    float scale, float* out, void* stream);

/* Inverse framed transform with windowed overlap-add:
 * out[b,m] = scale * sum_t w[q] y_t[q], q = m + crop_start - t*hop in [0,win),
 * y_t[n] = sum_k spec[b,t,k] cos(2pi/N (n+1/2+N/4)(k+1/2)).   spec [B,F,N/2] f32, out [B,out_len] f32.
 * IMDCT4.forward (mdct.py:542-566) = this with scale 4/N, crop_start = win/2 (center) and
 * out_len = min(out_length, (F-1)*hop [+win if !center]); the backward of MDCT4 = this with scale 1,
 * crop_start = start_pad, out_len = T. */
int p2phd_imdct4_fwd(const float* spec, int64_t B, int64_t n_frames, int n_fft, int hop, int win,
                     const float* window, const float* tables, int64_t crop_start, int64_t out_len,
                     float scale, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * MDCT2 / IMDCT2 and the DCT-II / DCT-III operators DCT_2N_native / IDCT_2N_native
 * (models/mdct.py:352-454, dct/dct_native.py:7-68; native counterparts dct/src/dct_2N_cuda.cpp,
 * dct_cuda_kernel.cu:267-406).  n_fft a power of two in [16, 2048]; tables as for MDCT4.
 *   forward  out[b,t,k] = scale * c_k * (2/N) * sum_i w[i] xpad[b, t*hop+i] cos(pi (2i+1) k / 2N), c_0 = k0_scale
 *   inverse  y_t[i]     = k0_scale * S[b,t,0] + 2 * sum_{k>=1} S[b,t,k] cos(pi (2i+1) k / 2N);
 *            out[b,m]   = scale * sum_t w[q] y_t[q], q = m + crop_start - t*hop in [0,win)
 * MDCT2.forward = forward(scale 1, k0 1); IMDCT2.forward = inverse(scale 1/2, k0 1); a plain DCT_2N_native on rows
 * [R,N] = forward with B = R, T = N, hop = win = N, window of ones, one frame per row (IDCT likewise);
 * autograd adjoints: forward^T = inverse(scale s/N, k0 2*k0), inverse^T = forward(scale s*N, k0 k0/2).
 * ---------------------------------------------------------------------------------------- */
size_t p2phd_dct_tables_floats(int n_fft);
int p2phd_dct_tables_fill(int n_fft, float* host_out);
int p2phd_mdct2_fwd(const float* x, int64_t B, int64_t T, int n_fft, int hop, int win, const float* window,
                    const float* tables, int64_t start_pad, int64_t n_frames, float scale, float k0_scale,
                    float* out, void* stream);
int p2phd_imdct2_fwd(const float* spec, int64_t B, int64_t n_frames, int n_fft, int hop, int win, const float* window,
                     const float* tables, int64_t crop_start, int64_t out_len, float scale, float k0_scale,
                     float* out, void* stream);
/* MDCT2.forward(signal, return_ola=True) (models/mdct.py:377-403): p2phd_mdct2_fwd plus a second output
 * frames[b,t,i] = w[i] * xpad[b, t*hop + i], i < win ([B, n_frames, win] f32): the windowed frame the kernel already holds
 * in LDS, written by the same launch.  `out` is bit-identical to p2phd_mdct2_fwd's. */
int p2phd_mdct2_fwd_frames(const float* x, int64_t B, int64_t T, int n_fft, int hop, int win, const float* window,
                           const float* tables, int64_t start_pad, int64_t n_frames, float scale, float k0_scale,
                           float* out, float* frames, void* stream);

/* ------------------------------------------------------------------------------------------
 * Time-domain discriminator (--use_time_D; pix2pixHD_model.py:251-258, 314-320, 375-387), csrc/timed.hip.
 *
 * p2phd_timed_pack_pair: the input of time_D's first conv.  lr_frames / other_frames: n_pixels f32 values each (a
 *   [N, F, win] tensor); dst: NHWC [N, F, win, 8] in `dtype`, channel 0 = lr, channel 1 = other, channels 2..7 zero.
 *   mode_db = 1: both through 20 log10(max(|x|, min_value)) - 20, i.e. aF.amplitude_to_DB(torch.abs(x), 20, min_value, 1)
 *   followed by torch.cat(dim=1) (discriminate_time_D, :314-320); mode_db = 0: the raw values (the generator-loss pass,
 *   torch.cat((lr_frames, sr_frames), dim=1) of :386).  dst 16-byte aligned.
 * p2phd_timed_frames_fwd: sr [B, 2, n_fft, n_frames] f32 (the generator's output), minmax = (min, max) of the low-rate
 *   clip's normalisation -> out[b,t,i] = scale * window[i] * IDCT_2N_native(S)[b,t,i], S[b,t,k] = (A0 - A1) / (2 alpha - 1),
 *   A_c = 10 * 10^((|sr[b,c,k,t]| (max - min) + min) / 20) - min_value: denormalize + to_frames (:229-232, :251-258) and
 *   the np.sqrt(up_ratio - 1) * window * . of :376 (scale = sqrt(up_ratio - 1), window of n_fft values).  tables:
 *   p2phd_dct_tables_fill(n_fft).  out [B, n_frames, n_fft] f32, 16-byte aligned.
 * p2phd_timed_frames_bwd: the adjoint.  g_frames [B, n_frames, n_fft] f32 (8-byte aligned), sr / minmax as in the
 *   forward -> g_sr [B, 2, n_fft, n_frames] = d<g_frames, out>/d sr (d|x|/dx = sign(x), 0 at 0; no gradient to minmax,
 *   which the reference computes under no_grad).
 * ---------------------------------------------------------------------------------------- */
int p2phd_timed_pack_pair(int dtype, const float* lr_frames, const float* other_frames, int64_t n_pixels, int mode_db,
                          float min_value, void* dst, void* stream);
int p2phd_timed_frames_fwd(const float* sr, const float* minmax, int64_t B, int64_t n_frames, int n_fft,
                           const float* window, const float* tables, float alpha, float min_value, float scale,
                           float* out, void* stream);
int p2phd_timed_frames_bwd(const float* g_frames, const float* sr, const float* minmax, int64_t B, int64_t n_frames,
                           int n_fft, const float* window, const float* tables, float alpha, float scale, float* g_sr,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Whole-file generation (pix2pixhdaudiosr_amd/generate/), csrc/stitch.hip.  Launch family "stitch".
 *
 * p2phd_segments_gather: audio [L] f32 -> out [S, T] f32, out[s,i] = audio[s * stride + i], zero beyond L.  1 <= stride <= T;
 *   stride = T is seg_pad_audio of the reference (data/audio_dataset.py:124-135).
 * p2phd_segments_stitch: seg [S, T] f32 -> out [L_out] f32 with V = T - stride shared samples between neighbours:
 *   out[n] = gain * sum_s w_s(n - s stride) seg[s, n - s stride] over the one or two segments that cover n.  w = 1 outside
 *   the overlaps; inside one the later segment has sin^2(pi (i + 1/2) / (2 V)) at its sample i < V and the earlier one
 *   1 - that value.  The first segment does not fade in, the last does not fade out.  V = 0: a scaled copy.  Evaluated in
 *   double, rounded once.  Errors (P2PHD_EINVAL): V outside [0, T/2], S < 1, L_out > (S - 1) stride + T.
 * p2phd_segments_gather_planar / p2phd_segments_stitch_planar: the same two over the C rows of a planar clip in ONE launch
 *   each (two "stitch" launches per clip whatever C is): audio [C][ld] -> out [C * S, T], channel-major (row c * S + s is
 *   segment s of channel c), and seg [C * S, T] -> out [C][ld], L_out samples per row, the rest of a row untouched.  Row c is
 *   bit-identical to the single-row entry on audio[c] / seg[c * S : (c + 1) * S].  Same errors, plus C < 1, ld < L, ld < L_out.
 * p2phd_segments_gather_ragged / p2phd_segments_stitch_ragged: the same two over N clip rows that share only T and stride -- the
 *   channels of several files -- in ONE launch each, one count of "stitch" per launch.  `table`, in HOST memory: N x 4 int64, row j
 *   = (address of audio_j resp. out_j on the device, L_j, S_j, row0_j); row j owns rows row0_j .. row0_j + S_j - 1 of seg [rows, T].
 *   The gather fills them from audio_j [L_j], the stitch writes out_j [L_j] from them; either is bit-identical to the planar entry
 *   on that clip alone (C = 1), and a row takes the 16-byte paths by its own base's alignment.  The entry checks the table before
 *   anything is launched (P2PHD_EINVAL): 1 <= N <= 65535; every L >= 0 and S >= 1; row0_0 = 0, row0_{j+1} = row0_j + S_j, the
 *   last row closing at `rows`; an address non-null where L > 0 and a multiple of 4; T, stride, V = T - stride and rows * T as
 *   above; stitch: L_j <= (S_j - 1) stride + T.  It then copies the checked table -- through pinned memory of its own, on `stream` --
 *   into `table_dev`, p2phd_segments_ragged_table_bytes(N) bytes on the device that the caller keeps alive until the launch has
 *   run, and the kernel reads that copy alone: what the caller does with `table` behind the call changes nothing.  Nothing is
 *   waited for.  Not inside a stream capture (P2PHD_EINVAL).  A stitch whose every L is 0 launches nothing.  Grid: blockIdx.y =
 *   clip row, grid.x from p2phd_stream_grid("segments_gather_ragged" / "segments_stitch_ragged") of the LONGEST row's outputs
 *   (S_j * T resp. L_j); a shorter row's surplus workgroups leave at once.
 * p2phd_segments_stitch_stream: the stitch of ONE WINDOW of a clip that goes through the pipeline in windows -- K consecutive
 *   segments s0 .. s0 + K - 1 of each of C channels, seg [C * K, T] channel-major -- in one launch, one count of "stitch".
 *   out[c * ld + n], 0 <= n < n_out <= (K - 1) stride + T, is the clip's stitched sample at position s0 stride + n: bit for bit
 *   row c of p2phd_segments_stitch_planar on the whole clip's segments there, for every n < K stride, and for every n where the
 *   window holds the clip's last segment (a sample at or beyond K stride of any other window also belongs to the segment behind
 *   it, which this call has not seen).  The window's segment 0 cross-fades with `carry_in` [C][V], V = T - stride: the raw,
 *   unscaled samples [stride, T) of each channel's segment s0 - 1, as the call on the window before left them in its `carry_out`.
 *   `first` != 0: the window holds the clip's segment 0, which does not fade in; carry_in is not read (it may be NULL).
 *   `carry_out` [C][V] receives this window's own tails, seg[c, K - 1, stride .. T); NULL: none are kept (the last window).  With
 *   V = 0 neither is read or written.  The same row body as every other stitch: the fp64 sine, one rounding.  Grid: blockIdx.y =
 *   channel, grid.x from p2phd_stream_grid("segments_stitch_stream") of n_out; a row takes the 16-byte paths by its own base in
 *   seg and out.  No atomics, no scratch, capturable, nothing is waited for.  Errors (P2PHD_EINVAL): K < 1, T < 1, V outside
 *   [0, T/2], C outside 1 .. 65535, n_out beyond the span, ld < n_out, first == 0 with V > 0 and carry_in NULL, carry_out
 *   overlapping carry_in, seg or out (two carry buffers take turns), seg or out NULL.  n_out = 0 launches nothing and leaves
 *   carry_out as it is.
 * ---------------------------------------------------------------------------------------- */
int p2phd_segments_gather(const float* audio, int64_t L, int64_t T, int64_t stride, int64_t S, float* out, void* stream);
int p2phd_segments_stitch(const float* seg, int64_t S, int64_t T, int64_t stride, float gain, float* out, int64_t L_out,
                          void* stream);
int p2phd_segments_gather_planar(const float* audio, int64_t C, int64_t ld, int64_t L, int64_t T, int64_t stride, int64_t S,
                                 float* out, void* stream);
int p2phd_segments_stitch_planar(const float* seg, int64_t C, int64_t S, int64_t T, int64_t stride, float gain, float* out,
                                 int64_t ld, int64_t L_out, void* stream);
int64_t p2phd_segments_ragged_table_bytes(int64_t N);      /* 32 * N; 0 for an N outside 1 .. 65535 */
int p2phd_segments_gather_ragged(const int64_t* table, int64_t N, int64_t T, int64_t stride, int64_t rows, float* seg, void* table_dev,
                                 void* stream);
int p2phd_segments_stitch_ragged(const float* seg, const int64_t* table, int64_t N, int64_t rows, int64_t T, int64_t stride, float gain,
                                 void* table_dev, void* stream);
int p2phd_segments_stitch_stream(const float* seg, int64_t C, int64_t K, int64_t T, int64_t stride, float gain, const float* carry_in,
                                 float* carry_out, int first, float* out, int64_t ld, int64_t n_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * PCM codec of whole-file generation, csrc/pcm.hip.  Launch family "pcm" (a decode and an encode count 1 each; frames = 0
 * launches nothing).  The payload is the little-endian INTERLEAVED sample stream of a RIFF data chunk (frame n, channel c at
 * sample n * channels + c); the float side is PLANAR, row c at c * ld, ld >= frames.  The payload pointer needs byte
 * alignment only.
 *
 * p2phd_pcm_decode: payload -> out[c * ld + n] f32, the scaling of data/wavio.py load and bit-identical to it: (u - 128) / 128
 *   for unsigned 8-bit, s / 2^(bits - 1) for signed 16 / 24 / 32-bit (one int -> float conversion, round to nearest even for
 *   32-bit, then an exact power-of-two scale), a bit copy for float32 (a NaN keeps its payload), round to nearest even for
 *   float64.
 * p2phd_pcm_encode: planar f32 -> payload.  P2PHD_PCM_S16 / _S24: clamp to [-1, (2^(bits-1) - 1) / 2^(bits-1)], times
 *   2^(bits-1), round half to even -- for PCM16 the bytes data/wavio.py save writes.  NaN encodes as 0 (wavio.save leaves
 *   that case undefined: the int16 conversion of a NaN is whatever the host gives).  P2PHD_PCM_F32: a bit copy.  Other
 *   formats: P2PHD_EINVAL.
 *
 * The output stage (opt-in; p2phd_pcm_encode is unchanged).  Each of the two counts 1 in the launch family "pcm".
 * p2phd_pcm_peak: what the encoder of `format` (P2PHD_PCM_S16 / _S24 / _F32) would meet in the rows of `planar` (layout and
 *   argument checks of p2phd_pcm_encode).  Per channel c: peak[c] = max |x| over the finite samples (0 for an empty row or one
 *   without a finite sample); over[c] = samples the encoder would clamp -- x > hi or x < -1 with hi = (2^(bits-1) - 1) / 2^(bits-1)
 *   for the integer formats, |x| > 1 for float32; +-inf counts, NaN does not; nonfinite[c] = NaN and +-inf samples.  And one gain
 *   for all channels (the stereo image is kept): with m = max_c peak[c], gain[0] = m > ceiling ? ceiling / m : 1 -- one fp32
 *   division; ceiling <= 0 stands for hi of the format (1 for float32).  All four are device pointers, written by every call
 *   (frames = 0 included) without having been zeroed, and hold the same bits on every run: a maximum of bit patterns and integer
 *   counts, folded by the last workgroup; no float atomics, no host synchronisation.  Like every fixed-order reduction of the
 *   library, two calls must be ordered (see "Streams" above).
 * p2phd_pcm_encode_ex: y = x * gain[0] (`gain`: device pointer, e.g. the one p2phd_pcm_peak wrote, read by the kernel; NULL: y = x).
 *   Integer formats: v = y * 2^(bits-1), v = v + d when dithering (one fp32 addition), r = rint(v) clamped to
 *   [-2^(bits-1), 2^(bits-1) - 1]; NaN -> 0.  float32 writes the bits of y.  dither: 0 = none, 1 = TPDF of +-1 LSB, P2PHD_PCM_S16
 *   only (with another format: P2PHD_EINVAL).  The dither of the interleaved sample with global index
 *   i = first_index + frame * channels + c (64-bit) is, in uint32 arithmetic,
 *     fmix(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16
 *     h = fmix(lo(i) ^ fmix(hi(i) ^ lo(seed) ^ 0x9E3779B9) ^ hi(seed))
 *     d = ((int)(h & 0xFFFF) - (int)(h >> 16)) * 2^-16            exact in fp32, in (-1, 1), triangular
 *   so a payload encoded in pieces (first_index = samples before the piece, >= 0) has the bytes of one call.  By construction
 *   (seed, i) = (0, 2^32) and (1, 0) draw the same value: harmless, the streams of two seeds are otherwise unrelated.
 *   gain = NULL and dither = 0: the bytes of p2phd_pcm_encode for every input (clamping before or after rounding gives the
 *   same codes).
 *
 * Big-endian containers (AIFF / AIFF-C, Sun/NeXT AU, NIST SPHERE; parsed by data/containers.py).  A file in one of the three
 * decodes to exactly the float32 samples data/wavio.py load returns for its WAV twin, the RIFF file that holds the same samples:
 *   integer PCM      the same width, little-endian, scaled by 2^-(8 * bytes - 1)
 *   signed 8-bit s   the twin holds s + 128: the value is s / 128
 *   float32          a bit copy after the byte swap; a NaN keeps its payload
 *   float64          rounded to nearest even, as P2PHD_PCM_F64
 *   G.711            the same bytes under format tags 6 / 7 (p2phd_g711_decode, "Coded WAV input" below), scaled as 16-bit PCM is
 * p2phd_pcm_decode_ex: p2phd_pcm_decode with `flags`, an OR of
 *   P2PHD_PCM_BIG_ENDIAN  the bytes of a sample stand most significant first (no effect with P2PHD_PCM_U8);
 *   P2PHD_PCM_SIGNED8     with P2PHD_PCM_U8 only: the byte is a two's-complement sample.
 *   flags = 0: the bits of p2phd_pcm_decode.  Layout, grid ("pcm_decode_ex" of p2phd_stream_grid) and argument checks are
 *   p2phd_pcm_decode's: 2, 4 and 8-byte samples are read with one typed load and byte-swapped where the payload pointer is aligned to
 *   the sample size and assembled byte-wise otherwise, 24-bit samples always byte-wise.  Counts 1 in "pcm"; frames = 0 launches
 *   and counts nothing.  P2PHD_PCM_SIGNED8 with another format, an unknown flag bit: P2PHD_EINVAL.
 * ---------------------------------------------------------------------------------------- */
#define P2PHD_PCM_U8  0   /* format tag 1,  8 bit */
#define P2PHD_PCM_S16 1   /* format tag 1, 16 bit */
#define P2PHD_PCM_S24 2   /* format tag 1, 24 bit */
#define P2PHD_PCM_S32 3   /* format tag 1, 32 bit */
#define P2PHD_PCM_F32 4   /* format tag 3, 32 bit */
#define P2PHD_PCM_F64 5   /* format tag 3, 64 bit */
int p2phd_pcm_decode(const void* bytes, int64_t frames, int channels, int format, float* out, int64_t ld, void* stream);
#define P2PHD_PCM_BIG_ENDIAN 1
#define P2PHD_PCM_SIGNED8    2   /* with P2PHD_PCM_U8 only: the byte is a two's-complement sample */
int p2phd_pcm_decode_ex(const void* bytes, int64_t frames, int channels, int format, int flags, float* out, int64_t ld, void* stream);
int p2phd_pcm_encode(const float* planar, int64_t frames, int channels, int64_t ld, int format, void* out, void* stream);
int p2phd_pcm_peak(const float* planar, int64_t frames, int channels, int64_t ld, int format, float ceiling, float* peak,
                   int64_t* over, int64_t* nonfinite, float* gain, void* stream);
int p2phd_pcm_encode_ex(const float* planar, int64_t frames, int channels, int64_t ld, int format, const float* gain, int dither,
                        uint64_t seed, int64_t first_index, void* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Time-domain crossover of whole-file generation, csrc/xover.hip.  Launch family "xover" (a p2phd_xover_fwd that launches
 * counts 1).  Below the crossover frequency the result is the input, above it the generator's output:
 *   out = sr + LP * (level * lr - sr)      ( = LP * (level * lr) + (delta - LP) * sr ),  LP a centred, zero-delay low-pass.
 *
 * p2phd_xover_taps_fill (HOST only, no device, as p2phd_resample_kernel_fill): the Kaiser-windowed sinc of `taps`
 *   coefficients (odd, 1 <= taps <= 4095) with its -6 dB point at `cutoff` cycles per sample (0 < cutoff < 0.5), beta >= 0.
 *   In float64, with n = k - (taps - 1) / 2 and sinc(x) = sin(pi x) / (pi x):
 *     h[k] = 2 cutoff sinc(2 cutoff n) I0(beta sqrt(1 - (2 n / (taps - 1))^2)) / I0(beta)
 *   divided by the float64 sum of all taps (DC gain 1), each tap then rounded once to fp32; h[k] and h[taps - 1 - k] hold the same
 *   bits.  taps = 1: h = [1].  Bad arguments: P2PHD_EINVAL with an error text.
 * p2phd_xover_fwd: sr, lr [C][ld_*] f32 (lr: the clip the generator was given, at the high rate and sample-aligned with sr),
 *   taps_dev: `taps` f32 coefficients on the device -- the caller's table, of any shape: symmetry is not assumed or used.
 *   With c0 = (taps - 1) / 2 and d[c][j] = level * lr[c][j] - sr[c][j] for 0 <= j < L, 0 outside (d is zero-extended, not the signals):
 *     out[c][i] = sr[c][i] + sum_{k = 0}^{taps - 1} h[k] d[c][i + c0 - k],     0 <= i < L.
 *   Arithmetic, fixed and independent of grid, tile and C: d is one rounded fp32 product and one rounded subtraction (NOT
 *   contracted); the sum is ONE fp32 accumulator that starts at +0 and takes acc = fma(h[k], d, acc) for k ascending (the
 *   products ARE contracted: one rounding per tap); then one rounded addition sr + acc.  So row c of a C-row call is bit for bit
 *   the 1-row call on that row, a run repeats bit for bit, and taps = 1 with h = [1] gives sr + (level * lr - sr) in fp32.
 *   Rows may start at any float, the pitches (>= L) are the caller's, all offsets are 64-bit.  `out` must not overlap sr or lr
 *   (the address spans of their C rows are compared): P2PHD_EINVAL.  Even taps, taps > 4095, C > 65535, a null or misaligned
 *   pointer: P2PHD_EINVAL.  L = 0 or C = 0: P2PHD_OK, nothing launched.  No atomics, no workspace.
 * p2phd_xover_tile_len (host): outputs per workgroup of p2phd_xover_fwd (tests place their lengths around it).
 * ---------------------------------------------------------------------------------------- */
int p2phd_xover_taps_fill(int taps, double cutoff, double beta, float* out);
int p2phd_xover_fwd(const float* sr, int64_t ld_sr, const float* lr, int64_t ld_lr, float level, const float* taps_dev, int taps,
                    int64_t C, int64_t L, float* out, int64_t ld_out, void* stream);
int p2phd_xover_tile_len(void);

/* ------------------------------------------------------------------------------------------
 * Spectrogram picture of whole-file generation, csrc/specimg.hip.  Launch family "specimg" (p2phd_stft_db and
 * p2phd_specimg_render count 1 each when they launch: 2 per picture).  Stacked panels, one per row of x, with one time axis
 * (the whole clip, left to right), one frequency axis (0 at a panel's bottom row, the Nyquist frequency at its top row) and one
 * dB scale.
 *
 * p2phd_specimg_tables_floats / _fill (HOST only): 3 n_fft floats -- tw[j] = exp(-2 pi i j / n_fft) as (cos, sin) pairs, then the
 *   periodic Hann window w[i] = 0.5 (1 - cos(2 pi i / n_fft)) -- float64 arithmetic, rounded once to fp32.  The caller uploads them.
 * p2phd_stft_db: x[R][ld] f32 rows of L samples (ld >= L; rows may start at any float; 64-bit offsets) -> db[R][F][K] f32,
 *   K = n_fft / 2 + 1, F = 1 + L / hop (integer division): the frames of
 *   torch.stft(x, n_fft, hop, window=hann_periodic, center=True, pad_mode='constant') -- frame f covers the samples
 *   f hop - n_fft / 2 .. + n_fft - 1, zero outside [0, L) --
 *     X[f][k] = sum_i w[i] x[f hop - n_fft / 2 + i] exp(-2 pi i k i / n_fft)
 *     P       = (re^2 + im^2) (4 / n_fft)^2          a full-scale sine reads 0 dB; the factor is an exact power of two
 *     db      = 10 log10f(max(P, 1e-20))             P <= 1e-20 is written as the constant -200: silence is one bit pattern
 *   n_fft: a power of two in [64, 2048]; 1 <= hop <= n_fft; R <= 65535; at most 2^30 frames; else P2PHD_EINVAL with an error
 *   text.  L = 0 or R = 0: P2PHD_OK, nothing launched.  Two neighbouring frames share one complex transform; no atomics, no
 *   reduction across workgroups: the same bits on every run.
 * p2phd_stft_db_frames (host): F for L >= 1 samples; 0 and an error text for arguments p2phd_stft_db would refuse (or L < 1).
 * p2phd_specimg_render: db[R][F][K] -> img[R H + (R - 1) gap][W][3] u8.  Pixel (panel r, row y, column x), all index arithmetic
 *   in integers with 64-bit products:
 *     y' = H - 1 - y
 *     frames f0 = floor(x F / W) .. f1 = max(f0 + 1, floor((x + 1) F / W))        (W > F repeats a frame, W < F pools)
 *     bins   k0 = floor(y' K / H) .. k1 = max(k0 + 1, floor((y' + 1) K / H))      (H > K repeats a bin,  H < K pools)
 *     v   = max of db[r][f][k] over f0 <= f < f1, k0 <= k < k1, folded with fmaxf from -inf (a NaN never wins)
 *     lo  = *top_dev - range                          top_dev: ONE f32 on the device, read by the kernel (no host round trip)
 *     t   = fmul_rn(v - lo, scale),  scale = 255 / range computed once on the host in fp32
 *     idx = clamp((int)rintf(t), 0, 255);  v = +inf: 255;  v = -inf (or nothing but NaN): 0;  a NaN t (NaN or infinite top): 0
 *     rgb = lut_dev[idx]                              lut_dev: 256 x 3 u8 on the device
 *   Every step is one correctly rounded fp32 operation or an exact function, so a float32 restatement gives the same bytes.
 *   The `gap` rows between two panels hold (64, 64, 64).  1 <= W, H <= 16384, 0 <= gap <= 64, range > 0 and finite, 1 <= K <= 4097,
 *   1 <= F <= 2^30, R <= 65535; else P2PHD_EINVAL.  R = 0: P2PHD_OK, nothing launched.  Every db value is read once.
 * p2phd_specimg_image_bytes (host): bytes of img for R >= 1 panels; 0 and an error text for bad arguments.
 * ---------------------------------------------------------------------------------------- */
size_t p2phd_specimg_tables_floats(int n_fft);
int p2phd_specimg_tables_fill(int n_fft, float* host_out);
int64_t p2phd_stft_db_frames(int64_t L, int n_fft, int hop);
size_t p2phd_specimg_image_bytes(int64_t R, int W, int H, int gap);
int p2phd_stft_db(const float* x, int64_t ld, int64_t R, int64_t L, int n_fft, int hop, const float* tables, float* db, void* stream);
int p2phd_specimg_render(const float* db, int64_t R, int64_t F, int K, const float* top_dev, float range, const uint8_t* lut_dev, int W,
                         int H, int gap, uint8_t* img, void* stream);

/* ------------------------------------------------------------------------------------------
 * Loudness of whole-file generation after ITU-R BS.1770-4 / EBU R 128, csrc/loudness.hip.  Launch family "loudness" (a
 * p2phd_loudness_hops that launches and every p2phd_loudness_gate count 1 each: 2 per measured clip; the loudness range, below, 2 more; the album loudness,
 * below them, 1 per clip and 1 per folder more).
 *
 * p2phd_loudness_coeffs_fill (HOST only, no device, as p2phd_xover_taps_fill): the K-weighting filter pair for `rate`, float64:
 *   out10 = b0 b1 b2 a1 a2 of the high shelf, then of the high-pass; y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2].
 *   Shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, K = tan(pi f0 / rate), Vh = 10^(G / 20),
 *   Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2; b0 = (Vh + Vb K / Q + K^2) / a0, b1 = 2 (K^2 - Vh) / a0,
 *   b2 = (Vh - Vb K / Q + K^2) / a0, a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0.  High-pass: f0 = 38.13547087602444,
 *   Q = 0.5003270373238773, the same K and a0 forms, b = (1, -2, 1), a1 and a2 as above.  At 48000 these are the coefficients
 *   printed in BS.1770 to 9e-16.  `rate` must be a multiple of 10 in [8000, 384000] (a hop is rate / 10 samples), else P2PHD_EINVAL.
 * p2phd_loudness_hops: planar [channels][ld] f32 rows of `frames` samples (layout and argument checks of p2phd_pcm_encode; rows
 *   may start at any float) -> z [channels][J] float64 on the device, hop = rate / 10, J = frames / hop (integer division; the
 *   samples behind J hop are not counted): z[c][j] = sum over the samples of hop j of y^2, y = row c through the shelf and then the
 *   high-pass from zero state at sample 0.  State and sums are float64, the samples are read as fp32.  Parallel by zero-state
 *   warm-up: hop j is computed from zero state at sample max(0, (j - 2) hop), 200 ms in front of it, and counts its own samples
 *   only -- hops 0 .. 2 are the sequential recursion, later ones lack a state response that has decayed by the high-pass's double
 *   pole over 200 ms (about 1e-17 of the state at any rate; below the float64 rounding of the recursion, 2^-53 / (1 - r)^2 = 4e-12).
 *   So a NaN or infinite sample reaches its own hop and the two behind it, not the rest of the clip.  Every z[c][j] is written by
 *   every call (nothing is zeroed before), by one work item in a fixed order: the same bits on every run, and row c of a
 *   C-row call holds the bits of the 1-row call on that row.  J = 0: P2PHD_OK, nothing launched.  No atomics, no workspace.
 * p2phd_loudness_gate: z [channels][J] (device) -> res4 (4 float64, device) and gain (1 f32, device), one workgroup, fixed-order
 *   float64 sums; always launches.  weights: HOST pointer to `channels` f32 (finite, >= 0; NULL: all 1); 1 <= channels <= 64.
 *     blocks   NB = max(J - 3, 0); P[c][b] = (((z[c][b] + z[c][b+1]) + z[c][b+2]) + z[c][b+3]) / (4 hop);
 *              p[b] = sum_c weights[c] P[c][b], c ascending from 0; l[b] = -0.691 + 10 log10(p[b])
 *     gating   A = {b : l[b] > -70};  Gamma = -0.691 + 10 log10(mean_A p) - 10;  B = {b in A : l[b] > Gamma};
 *              I = -0.691 + 10 log10(mean_B p).  Both comparisons are evaluated as "not l <= threshold": a block whose level is NaN
 *              stays in, so a NaN in z makes I NaN instead of being gated out.
 *     res4     {I, max_b l[b] (fmax from -inf: a NaN never wins), Gamma, |B|}; with NB = 0 or A empty {-inf, -inf or the maximum, -inf, 0}
 *     gain     T = *target_dev where target_dev != NULL (a device float64, e.g. another clip's res4: no host round trip), else
 *              `target`; gain[0] = (float) 10^(clamp(T - I, -max_gain_db, +max_gain_db) / 20), float64 arithmetic rounded once;
 *              gain[0] = 1 where T or I is not finite (target NaN: no target).  max_gain_db finite and >= 0.
 *
 * Loudness range after EBU Tech 3342 and the maximum short-term loudness, from the same z (1 launch each, family "loudness"):
 * p2phd_loudness_short_term: z [channels][J] (device) -> p [NS] float64 (device), NS = max(J - 29, 0): the power of the 3 s block of
 *   hops b .. b + 29 (100 ms step).  S[c] = ((z[c][b] + z[c][b+1]) + ..) + z[c][b+29], left to right, every block on its own (no
 *   running sum: the bits of p[b] do not depend on b); P[c] = S[c] / (30.0 hop); p[b] = sum_c weights[c] P[c], c ascending from 0;
 *   p[b] = p[b] (g g), g = (double) gain_dev[0], where gain_dev != NULL (one f32 on the DEVICE, read by the kernel: a gate's gain,
 *   no host round trip).  Nothing contracted; one writer per element.  weights, channels, rate, J: as p2phd_loudness_gate.
 *   NS = 0: P2PHD_OK, nothing launched.
 * p2phd_loudness_range: p [NS] (device, read only; non-negative or NaN) -> res8 (8 float64, device), one workgroup; always launches.
 *     gating   A = {b : p[b] > 1.1724653045822981e-07} (-70 LUFS as a power);  m = mean_A p (fixed-order sum);
 *              B = {b in A : p[b] > 0.01 m} (20 LU under the mean).  A power equal to a threshold is out, and so is a NaN.
 *     ranks    n = |B|, q = B's powers ascending; k_lo = ((n - 1) 10 + 50) / 100, k_hi = ((n - 1) 95 + 50) / 100 (integer division):
 *              the round((n - 1) PRC / 100 + 1) of the Tech 3342 reference code, zero-based.  q[k] is the exact order statistic
 *              (MSB-first radix select on the bit patterns, integer counts in LDS): no sort buffer, no workspace, no float atomics.
 *     res8     {LRA = lufs(q[k_hi]) - lufs(q[k_lo]), lufs(q[k_lo]), lufs(q[k_hi]), lufs(0.01 m) (-inf with A empty), n,
 *              lufs(max_b p[b]) (fmax from 0: a NaN never wins; -inf with NS = 0), q[k_lo], q[k_hi]}, lufs(x) = -0.691 + 10 log10(x).
 *              n = 0: {0, -inf, -inf, .., 0, .., 0, 0}.  Any p[b] NaN: LRA, both levels and both powers are NaN (a broken clip shows);
 *              the threshold, n and the maximum are those of the other blocks.  +inf is a value like any other: it makes m infinite,
 *              so nothing is over 0.01 m and n = 0.  The same bits on every run and on every stream.
 *
 * Album loudness (EBU R 128: a folder as one programme), from the same z (1 launch each, family "loudness"):
 * p2phd_loudness_blocks: z [channels][J] (device) -> p [NB] float64 (device), NB = max(J - 3, 0): p[b] of p2phd_loudness_gate's
 *   "blocks" line, the very expression (one device function serves both), so p[b] holds the bits the gate computes in place.  `p`
 *   is where the caller points: a slice of a buffer that takes the blocks of every file of a folder, one file behind the other -- a
 *   block never spans two files.  Grid-parallel, one writer per element, nothing contracted; elements outside [0, NB) are not
 *   touched.  weights, channels, rate, J: as p2phd_loudness_gate.  J < 4: P2PHD_OK, nothing launched.
 * p2phd_loudness_gate_blocks: p [NB] (device, read only) -> res4 and gain as p2phd_loudness_gate leaves them ("gating", "res4",
 *   "gain" above, with l[b] = -0.691 + 10 log10(p[b])); always launches.  One workgroup of 256: thread t sums the blocks t, t + 256,
 *   .. in ascending order and the partial sums meet in the gate's tree -- both entries run one body -- so on the p of one file it
 *   returns the bits p2phd_loudness_gate returns on that file's z, and on a folder's p the sums have one fixed order.  No atomics,
 *   no workspace, the same bits on every run and on every stream.  The price of the one workgroup: the time grows with NB / 256
 *   dependent steps of one compute unit (two passes over p) where a grid-wide fold would use the whole device.
 * ---------------------------------------------------------------------------------------- */
int p2phd_loudness_coeffs_fill(double rate, double* out10);
int p2phd_loudness_hops(const float* planar, int64_t frames, int channels, int64_t ld, int rate, double* z, void* stream);
int p2phd_loudness_gate(const double* z, int64_t J, int channels, int rate, const float* weights, double target, const double* target_dev,
                        double max_gain_db, double* res4, float* gain, void* stream);
int p2phd_loudness_short_term(const double* z, int64_t J, int channels, int rate, const float* weights, const float* gain_dev, double* p,
                              void* stream);
int p2phd_loudness_range(const double* p, int64_t NS, double* res8, void* stream);
int p2phd_loudness_blocks(const double* z, int64_t J, int channels, int rate, const float* weights, double* p, void* stream);
int p2phd_loudness_gate_blocks(const double* p, int64_t NB, double target, const double* target_dev, double max_gain_db, double* res4,
                               float* gain, void* stream);

/* ------------------------------------------------------------------------------------------
 * Active speech level of whole-file generation after ITU-T P.56 method B, csrc/speechlevel.hip.  Launch family "speechlevel":
 * p2phd_speechlevel_envelope, p2phd_speechlevel_counts and p2phd_speechlevel_decide with frames > 0 count 1 each, 3 per measured
 * clip, 6 per file (the clip the generator was given and the generated one).  The procedure is method B as the speech voltmeter
 * of the ITU-T Software Tool Library implements it, WRITTEN FROM MEMORY (the Recommendation's text was not at hand), with a linear
 * interpolation in dB where the tool bisects to 0.5 dB.  No 200 .. 5500 Hz weighting, no DC figure, no method A.
 *
 * Units: levels are in dBov for samples in [-1, 1): 10 log10(mean x^2); a full-scale sine reads -3.01.  P.56 is defined on one
 * channel: every row is measured on its own.  The file's figure is that of the channel with the highest finite active level, the
 * lowest channel index on a tie (no finite level: the first channel whose level is not -inf, else channel 0); one gain applies
 * to all channels.  A file whose channels all have no activity has the level -inf and the gain 1.
 *
 * Constants, all float64, f = the rate, an int in 8000 .. 192000: g = exp(-1 / (0.03 f)); h = 1 - g; I = ceil(0.2 f) = (f + 4) / 5
 * in integers; M = 15.9; the 15 thresholds c_j = 2^(j - 15), j = 0 .. 14; L = 256; gL = g squared eight times; hL = (256 h) gL.
 * p2phd_speechlevel_consts_fill (HOST only): out8 = {g, h, gL, hL, M, c_0, L, I}, *hang = I; rate outside the range: P2PHD_EINVAL.
 *
 * Envelope: r_i = |x_i| (fp32 to float64, exact); p_i = (g p_{i-1}) + (h r_i); q_i = (g q_{i-1}) + (h p_i): every operation a
 * separate IEEE double multiply or add, nothing contracted.  The parallel order is the contract.  Chunk k holds the samples
 * [k L, k L + L), the last may be shorter.
 *   1. the recursion from (0, 0) over each full chunk -> (zp_k, zq_k);
 *   2. left to right over the chunks: P_0 = Q_0 = 0; Q_{k+1} = ((gL Q_k) + (hL P_k)) + zq_k; P_{k+1} = (gL P_k) + zp_k;
 *   3. the recursion over each chunk again from (P_k, Q_k) -> q_i.
 * Threshold index: m_i = the number of j with q_i >= c_j, a uint8 in 0 .. 15; a NaN q gives 0.
 * Energy: s_k = the sum of x_i^2 over chunk k, left to right (each product exact in float64); sq = the sum of s_k, left to right.
 * Activity: tm_i = max(m_{max(0, i - I)} .. m_i); a_j = #{i : tm_i > j}, int64 -- the 200 ms hangover counters of P.56 exactly
 * (the thresholds are nested, so the trailing maximum of the index is the hangover of all of them).
 * Decision, n frames: long_term = 10 log10(sq / n); for j with a_j > 0: A_j = 10 log10(sq / a_j), D_j = A_j - 20 log10(c_j).
 *   a_0 = 0: no activity, the level is -inf, the activity 0, the bracket -1.  Otherwise the first j with D_j <= M: j = 0 gives A_0,
 *   j > 0 gives A = A_{j-1} + t (A_j - A_{j-1}), t = (D_{j-1} - M) / (D_{j-1} - D_j); no such j before a_j = 0 or j = 15: the last
 *   valid A_j (the bracket is that j).  activity = 10^((long_term - A) / 10).  A non-finite sq gives a non-finite level.
 * Gain: T = *target_dev where target_dev != NULL (a device float64, e.g. the file figure of another clip's res: no host round
 *   trip), else `target`; gain[0] = (float) 10^(clamp(T - A_file, -max_gain_db, +max_gain_db) / 20), float64 arithmetic rounded
 *   once; gain[0] = 1 where T or A_file is not finite (target NaN: no target).  max_gain_db finite and >= 0.
 *
 * p2phd_speechlevel_workspace_bytes (host): bytes of the envelope's workspace, channels * ceil(frames / 256) * 24; 0 for frames <= 0.
 * p2phd_speechlevel_tile_len (host): samples per workgroup tile of the envelope's and the counts' grids (16384).
 * p2phd_speechlevel_envelope: planar [channels][ld] f32 rows (layout and checks of p2phd_pcm_encode; 1 <= channels <= 64; rows may
 *   start at any float) -> m [channels][ld_m] uint8 (bytes behind `frames` of a row are not touched) and sq [channels] float64, on
 *   the device; `workspace`: the caller's, of the queried size, 8-byte aligned, every byte the call reads it has written before;
 *   after the call it holds, per row, P_k, Q_k and s_k as three float64 arrays of ceil(frames / 256) (what the tests compare bit for bit).
 *   Three kernels behind one another on the stream (steps 1, 2, 3), counted as one launch.  frames = 0: P2PHD_OK, nothing launched.
 * p2phd_speechlevel_counts: m -> a [channels][16] int64 (device), zeroed by the entry on the stream; a[c][15] is unused padding
 *   and stays 0.  Integer counts met by integer atomics: the same bits on every run.  frames = 0: a is zeroed, nothing launched.
 * p2phd_speechlevel_decide: sq, a -> res [(channels + 1)][4] float64 and gain (1 f32), device; one workgroup, always launches.
 *   Row c = {active level, long-term level, activity, bracket j}; row `channels` = the file's figure {active, long-term, activity,
 *   channel index}.  frames = 0: every row {-inf, -inf, 0, -1}, the file's {.., 0}, gain 1.
 * The grids are capped at 2048 workgroups per row and walk the tiles beyond with their stride ("speechlevel_grid" of
 * p2phd_set_option lowers the cap); the result's bits depend on neither.  No float atomics, no scratch, nothing waits on the host.
 * ---------------------------------------------------------------------------------------- */
int p2phd_speechlevel_consts_fill(int rate, double* out8, int* hang);
size_t p2phd_speechlevel_workspace_bytes(int64_t frames, int channels);
int p2phd_speechlevel_tile_len(void);
int p2phd_speechlevel_envelope(const float* planar, int64_t frames, int channels, int64_t ld, int rate, uint8_t* m, int64_t ld_m, double* sq,
                               void* workspace, void* stream);
int p2phd_speechlevel_counts(const uint8_t* m, int64_t frames, int channels, int64_t ld_m, int rate, int64_t* a, void* stream);
int p2phd_speechlevel_decide(const double* sq, const int64_t* a, int64_t frames, int channels, double target, const double* target_dev,
                             double max_gain_db, double* res, float* gain, void* stream);

/* ------------------------------------------------------------------------------------------
 * True peak of whole-file generation after ITU-R BS.1770-4 Annex 2 (oversample, take the largest magnitude), csrc/truepeak.hip.
 * Launch family "truepeak" (a p2phd_truepeak with frames > 0 counts 1).
 *
 * p2phd_truepeak_taps_fill (HOST only, no device, as p2phd_xover_taps_fill): the polyphase table c[factor][P], phase-major, of a
 *   Kaiser-windowed sinc interpolator; factor F = 1, 2 or 4, P = taps_per_phase even and in [4, 64], beta finite and >= 0.  In
 *   float64, with tau = (k - (P / 2 - 1)) - p / F and sinc(x) = sin(pi x) / (pi x):
 *     c[p][k] = sinc(tau) I0(beta sqrt(1 - (tau / (P / 2))^2)) / I0(beta)
 *   each phase divided by its own float64 sum (DC gain 1), each coefficient then rounded once to fp32.  Phase 0 is written as the
 *   unit impulse at k = P / 2 - 1, not computed.  c[p][k] and c[F - p][P - 1 - k] are written from one value: the same bits.  Bad
 *   arguments: P2PHD_EINVAL with an error text.
 * p2phd_truepeak: planar [channels][ld] f32 rows of `frames` = L samples (layout and argument checks of p2phd_pcm_peak; rows may
 *   start at any float), table_dev: factor * P f32 on the device -- the caller's table, of any shape: neither the symmetry nor the
 *   impulse of phase 0 is assumed or used (phase 0 is not read).  x~ is the row, 0 outside [0, L), every NaN or infinite sample taken
 *   as 0 (p2phd_pcm_peak counts those).  For p = 1 .. F - 1 and i = -1 .. L - 1
 *     y[i][p] = sum_{k = 0}^{P - 1} c[p][k] x~[i + k - (P / 2 - 1)]
 *   as ONE fp32 accumulator that starts at +0 and takes acc = fma(c[p][k], x~, acc) for k ascending (one rounding per tap), so a
 *   y has one bit pattern whatever the grid, the tile and the number of rows.  Phase 0 is not computed: it is |x~[i]|, i = 0 .. L - 1.
 *   tpeak[c] = the maximum of all these magnitudes of row c, as a maximum of bit patterns: tpeak[c] >= the peak[c] of
 *   p2phd_pcm_peak, always.  gain[0] = m > ceiling ? ceiling / m : 1 with m = max_c tpeak[c], one fp32 division: one gain for all
 *   channels.  ceiling: finite and > 0.  Both outputs are device pointers, written by every call (frames = 0 included: zeros and
 *   gain 1, not counted as a launch) without having been zeroed, and hold the same bits on every run: workgroup maxima folded by
 *   the last workgroup; no float atomics, no host synchronisation, no workspace.  Like every fixed-order reduction of the library,
 *   two calls must be ordered (see "Streams" above).  A bad factor or P, ceiling <= 0, a null or misaligned pointer, ld < frames:
 *   P2PHD_EINVAL.
 * p2phd_truepeak_tile_len (host): instants per workgroup tile of p2phd_truepeak (tests place their lengths around it).
 * ---------------------------------------------------------------------------------------- */
int p2phd_truepeak_taps_fill(int factor, int taps_per_phase, double beta, float* out);
int p2phd_truepeak(const float* planar, int64_t frames, int channels, int64_t ld, const float* table_dev, int factor, int taps_per_phase,
                   float ceiling, float* tpeak, float* gain, void* stream);
int p2phd_truepeak_tile_len(void);

/* ------------------------------------------------------------------------------------------
 * Look-ahead true-peak limiter of whole-file generation, csrc/limiter.hip (the definition is that file's header comment).
 * Launch family "limiter": p2phd_limiter_envelope and p2phd_limiter_apply with frames > 0 count 1 each, 2 per clip.
 *
 * p2phd_limiter_window_fill (HOST only, no device): the smoothing window w[0 .. A], A = lookahead in [1, 1024], A + 1 floats:
 *   in float64 w[k] = 0.5 - 0.5 cos(2 pi (k + 1) / (A + 2)), divided by the float64 sum, each rounded once to fp32; w[k] and w[A - k]
 *   are written from one value: the same bits.
 * p2phd_limiter_envelope: planar, frames, channels, ld, table_dev, factor, taps_per_phase, ceiling as p2phd_truepeak takes them.
 *   r_out[frames] f32 on the device: r[i] = m[i] > ceiling ? ceiling / m[i] : 1 with m[i] the largest, over the channels, of
 *   |x~[i]| and the fractional phases |y[i][p]|, |y[i - 1][p]| on both sides of sample i -- every y with the bits p2phd_truepeak
 *   forms.  peak_in_out (one f32 on the device, written, not read): the largest m, which is the largest tpeak p2phd_truepeak
 *   reports for the clip, bit for bit; 0 for frames = 0.  Maxima of bit patterns folded by the last workgroup: no float atomics,
 *   nothing is zeroed beforehand, no host synchronisation.
 * p2phd_limiter_apply: r[frames] f32 on the device (the envelope's, or any values in (0, 1]; taken as 1 outside [0, frames)),
 *   lookahead A in [1, 1024], hold H in [0, 4096], window_dev: A + 1 f32 on the device (any values: neither the symmetry nor the
 *   sum is assumed).  h[j] = min r[j - H .. j + A], d = 1.0f - h, s[i] = sum_k window[k] d[i - k] (one fp32 accumulator from +0, fma
 *   in ascending k), g[i] = min(r[i], 1.0f - s[i]); out[c][i] = planar[c][i] * g[i] for every channel, rows out_ld apart (out may
 *   not overlap planar); g_out: NULL, or frames f32 that take g.  stats_out: 8 bytes on the device -- the smallest g as f32 (1 where
 *   nothing is reduced), then the number of i with g[i] < 1 as u32 (saturating) -- folded in a fixed order in the same launch.
 *   A tile whose r within reach are all 1 copies its samples: the same bits as the multiply gives a finite sample.
 *   frames = 0 is valid: the statistics are 1 and 0.
 * Both share one region of the reduction scratch: the two calls (and any two calls of the family) must be ordered (see "Streams").
 * A bad factor, P, lookahead or hold, ceiling <= 0, a null or misaligned pointer, ld < frames: P2PHD_EINVAL, nothing is launched.
 * p2phd_limiter_tile_len (host): samples per workgroup tile of p2phd_limiter_apply; the envelope lays its tiles one sample closer
 *   (tile_len - 1 apart), because a sample needs the instants on both of its sides.
 * ---------------------------------------------------------------------------------------- */
int p2phd_limiter_window_fill(int lookahead, float* out);
int p2phd_limiter_envelope(const float* planar, int64_t frames, int channels, int64_t ld, const float* table_dev, int factor, int taps_per_phase,
                           float ceiling, float* r_out, float* peak_in_out, void* stream);
int p2phd_limiter_apply(const float* planar, int64_t frames, int channels, int64_t ld, const float* r, int lookahead, int hold,
                        const float* window_dev, float* out, int64_t out_ld, float* g_out, void* stats_out, void* stream);
int p2phd_limiter_tile_len(void);

/* ------------------------------------------------------------------------------------------
 * Effective bandwidth of whole-file generation, csrc/bandwidth.hip: where the band of a clip ends, read off its long-term average
 * spectrum.  Launch family "bandwidth": p2phd_ltas counts 1 when F > 0 and R > 0, p2phd_bandwidth 1 when G > 0 -- 2 per clip.
 *
 * p2phd_ltas_frames (host): F = 1 + (L - n_fft) / hop for L >= n_fft, else 0 -- only the frames that lie wholly inside the clip,
 *   frame f covering samples f hop .. f hop + n_fft - 1: torch.stft(center=False) with the periodic Hann window.  (Not the
 *   center=True frames of p2phd_stft_db: the step under the window of a zero-padded edge frame leaks into every bin, and that floor
 *   decides where a band seems to end.)  -1 and an error text for arguments p2phd_ltas would refuse.
 * p2phd_ltas_chunk_frames (host): a compile-time constant, the frames of one chunk.
 * p2phd_ltas_workspace_bytes (host): bytes of the workspace of a call, R * ceil(F / chunk) * K float64; 0 where F = 0 or R = 0 (and,
 *   with an error text, for arguments p2phd_ltas would refuse).
 * p2phd_ltas: x[R][ld] f32 rows of L samples (ld >= L; rows may start at any float; 64-bit offsets) -> psd[R][K] float64,
 *   K = n_fft / 2 + 1.  Per frame and bin P = (re^2 + im^2) (4 / n_fft)^2 in fp32 -- the value p2phd_stft_db takes the logarithm
 *   of: window and twiddles from the caller's `tables` (p2phd_specimg_tables_fill, n_fft of them on the device), two neighbouring
 *   frames of a chunk through one complex transform.  psd[r][k] is the float64 sum of the frames' P (each P widened exactly) in one
 *   fixed order: frames are taken in chunks of p2phd_ltas_chunk_frames() consecutive frames; a chunk's sum starts at +0 and takes
 *   its frames in ascending order; the row's sum starts at +0 and takes the chunks' sums in ascending order.  One workgroup per
 *   (row, chunk) keeps its bins' sums in float64 registers and stores one partial [K] into `workspace`; the last workgroup of a row
 *   to arrive (an integer ticket of the library's reduction scratch, fence then atomic; see "Streams": two calls must be ordered)
 *   folds the row's partials.  No float atomics, nothing is zeroed beforehand, one launch.  Row r of an R-row call holds the bits of
 *   the one-row call on that row, and a run repeats bit for bit.  F = 0: psd is zero-filled (hipMemsetAsync, not counted), P2PHD_OK.
 *   n_fft a power of two in [64, 2048], 1 <= hop <= n_fft, 0 <= R <= 65535, 0 <= L <= 2^40, F <= 2^30, psd and workspace aligned
 *   to 8 bytes, x to 4, tables to 8: anything else is P2PHD_EINVAL with an error text, nothing launched.
 * p2phd_bandwidth: psd[G Q][K] float64 (device) -> res[G][4] float64 (device), one workgroup per group, all arithmetic float64 in
 *   the order written here, nothing contracted, so that a restatement on the host returns the same bits:
 *     group    s[k] = ((psd[g Q][k] + psd[g Q + 1][k]) + ..) + psd[g Q + Q - 1][k]: the Q rows of a group (the channels of a clip)
 *              are one programme, as with loudness
 *     bands    band b covers the bins [b M, min(K, (b + 1) M)), M = band_bins; its level is ((s[b M] + s[b M + 1]) + ..) divided
 *              by its bin count (one division)
 *     ref      the largest band level: from 0.0, `if (level > ref) ref = level` over the bands -- a NaN (or a negative level)
 *              never wins
 *     thr      ref * rel, one rounded product; rel = 10^(-threshold_db / 10) is computed once on the host and passed as a double
 *     b_top    the highest band with level > thr (strictly; a NaN fails)
 *     k_top    the highest bin of band b_top with s[k] > thr -- one exists, since the band's mean is above thr
 *     res      {k_top, b_top, ref, thr}; {-1, -1, ref, thr} when no band passes: silence (ref = 0), all NaN, an infinite level
 *   No workspace, no atomics, one launch.  1 <= K <= 4097, 1 <= M <= K, Q >= 1, 0 <= G, G Q <= 2^31 - 1, rel finite and in (0, 1]:
 *   anything else is P2PHD_EINVAL with an error text.  G = 0: P2PHD_OK, nothing launched.
 * ---------------------------------------------------------------------------------------- */
int64_t p2phd_ltas_frames(int64_t L, int n_fft, int hop);
int p2phd_ltas_chunk_frames(void);
size_t p2phd_ltas_workspace_bytes(int64_t R, int64_t L, int n_fft, int hop);
int p2phd_ltas(const float* x, int64_t ld, int64_t R, int64_t L, int n_fft, int hop, const float* tables, double* psd, void* workspace,
               void* stream);
int p2phd_bandwidth(const double* psd, int64_t G, int Q, int K, int band_bins, double rel, double* res, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stereo image of whole-file generation, csrc/stereo.hip: how the two channels of a clip relate below and above a split bin, read
 * off their long-term cross-spectrum, and the mid/side matrix of SuperResolver(stereo='ms').  Launch family "stereo": p2phd_xspec
 * counts 1 when F > 0 and G > 0, p2phd_stereo_bands 1 when G > 0 (2 per measured clip), p2phd_stereo_matrix 1 when L > 0 (2 per
 * clip generated as mid / side: the encoder and the decoder).
 *
 * p2phd_xspec_workspace_bytes (host): bytes of the workspace of a call, G * ceil(F / chunk) * 4 * K float64 -- four times
 *   p2phd_ltas's per row pair; F = p2phd_ltas_frames(L, n_fft, hop), chunk = p2phd_ltas_chunk_frames().  0 where F = 0 or G = 0 (and,
 *   with an error text, for arguments p2phd_xspec would refuse).
 * p2phd_xspec: x[2 G][ld] f32 rows of L samples (ld >= L; rows may start at any float; 64-bit offsets); rows 2 g and 2 g + 1 are the
 *   left and the right channel of pair g -> xs[G][4][K] float64, K = n_fft / 2 + 1.  With A and B the transforms of the two
 *   channels' Hann-windowed frame (p2phd_ltas's frames -- only those wholly inside the clip --, window, `tables` and (4 / n_fft)^2
 *   scale; both channels of a frame through one complex transform, z = w x_L + i w x_R), per frame and bin in fp32:
 *     row 0  |A|^2        row 1  |B|^2        row 2  Re(A conj B)        row 3  Im(A conj B)
 *   xs[g][q][k] is the float64 sum of the frames' values (each widened exactly) in p2phd_ltas's fixed order: chunks of
 *   p2phd_ltas_chunk_frames() consecutive frames, each summed from +0 ascending, the chunks' sums added from +0 ascending.  One
 *   workgroup per (pair, chunk) stores one partial [4][K] into `workspace`; the last workgroup of a pair to arrive folds the pair's
 *   partials, one of the four rows at a time.  The arrival tickets are those of p2phd_ltas (FOLD_LTAS, the tickets-only region of
 *   the library's reduction scratch; see "Streams": a p2phd_ltas and a p2phd_xspec on two streams are ordered like two calls of
 *   either).  No float atomics, nothing is zeroed beforehand, one launch.  Pair g of a G-pair call holds the bits of the one-pair
 *   call on that pair, and a run repeats bit for bit.  F = 0: xs is zero-filled (hipMemsetAsync, not counted), P2PHD_OK.  G = 0:
 *   P2PHD_OK, nothing launched.  n_fft a power of two in [64, 2048], 1 <= hop <= n_fft, 0 <= G <= 32767, 0 <= L <= 2^40, F <= 2^30,
 *   xs and workspace aligned to 8 bytes, x to 4, tables to 8: anything else is P2PHD_EINVAL with an error text, nothing launched.
 * p2phd_stereo_bands: xs[G][4][K] float64 (device) -> res[G][8] float64 (device) = {S_ll, S_rr, Re, Im} of the band [0, k_split),
 *   then of the band [k_split, K): 64 bytes per pair, one workgroup of 256 lanes per pair.  Each of the eight sums over its band
 *   [lo, hi) of its row v is float64 in this order, nothing contracted, so that a restatement on the host returns the same bits:
 *     lanes    lane t (0 .. 255) starts at +0.0 and adds v[lo + t], v[lo + t + 256], v[lo + t + 512], .. below hi, ascending
 *     tree     for o = 128, 64, .. 1: lane t < o takes s[t] = s[t] + s[t + o]; the sum is s[0]
 *   NaN and infinity go through as IEEE arithmetic leaves them.  2 <= K <= 4097, 1 <= k_split <= K - 1, 0 <= G, pointers aligned to
 *   8 bytes: anything else is P2PHD_EINVAL with an error text.  G = 0: P2PHD_OK, nothing launched.  No workspace, no atomics.
 * p2phd_stereo_matrix: x[2][ld] f32 -> out[2][ld_out] f32, L samples a row: out0[i] = a * (x0[i] + s), out1[i] = a * (x0[i] - s) with
 *   s = x1[i]; with guard_side != 0 a non-finite x1[i] (NaN, +inf, -inf) is read as +0 -- "no side here" -- while a non-finite
 *   x0[i] stays what it is.  Plain fp32, one rounding per operation (one sum or difference, one product), nothing contracted: numpy
 *   float32 repeats it bit for bit.  a = 0.5 without the guard is the encoder (mid, side) = ((L + R) / 2, (L - R) / 2), a = 1 with
 *   the guard the decoder (L, R) = (M + S, M - S).  Grid-stride, float4 where both pointers are aligned to 16 bytes and both
 *   pitches are multiples of 4, one launch.  In place is allowed as out == x with ld_out == ld; any other overlap of the two
 *   buffers is refused.  ld, ld_out >= L, 0 <= L <= 2^40, a finite, pointers aligned to 4 bytes: anything else is P2PHD_EINVAL with
 *   an error text.  L = 0: P2PHD_OK, nothing launched.
 * ---------------------------------------------------------------------------------------- */
size_t p2phd_xspec_workspace_bytes(int64_t G, int64_t L, int n_fft, int hop);
int p2phd_xspec(const float* x, int64_t ld, int64_t G, int64_t L, int n_fft, int hop, const float* tables, double* xs, void* workspace,
                void* stream);
int p2phd_stereo_bands(const double* xs, int64_t G, int K, int k_split, double* res, void* stream);
int p2phd_stereo_matrix(const float* x, int64_t ld, int64_t L, float a, int guard_side, float* out, int64_t ld_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rate converter of whole-file generation's output stage (--output_rate), csrc/rateconv.hip: a rational polyphase FIR from the
 * model's rate to the rate that is written.  Launch family "rateconv" (a p2phd_rateconv_fwd with frames > 0 counts 1).  It is not the
 * feeder's p2phd_resample_fwd, which restates the reference's training-time resampler and stays as it is.
 * With g = gcd(in_rate, out_rate): o = in_rate / g, n = out_rate / g, P = taps_per_phase, half = P / 2 - 1.
 *
 * p2phd_rateconv_plan (HOST only, no device, as p2phd_xover_taps_fill): the filter for a passband and an attenuation, in float64.
 *   nyq = min(in_rate, out_rate) / 2, fp = passband * nyq (flat up to here), fs = 2 nyq - fp (the stopband from here: aliases and
 *   images fold only above fp), beta = 0.1102 (atten_db - 8.7), and Kaiser's length
 *     P = 2 ceil((atten_db - 7.95) / (2 * 2.285 * 2 pi (fs - fp) / in_rate)).
 *   Refused (P2PHD_EINVAL with an error text): in_rate == out_rate, a rate < 1, passband outside (0, 1), atten_db outside [40, 160],
 *   P < 4 or P > 256, n * P > 2^20.  generate/plans.py holds the defaults (passband 0.907: 20 kHz at 44.1 kHz; 120 dB).
 * p2phd_rateconv_taps_fill (HOST only): the table c[n][P], phase-major.  Phase p has frac = ((p o) mod n) / n; in float64, with
 *   tau = (k - half) - frac, sinc(x) = sin(pi x) / (pi x) and cutoff = fc = 2 nyq / in_rate in (0, 1]:
 *     c[p][k] = fc sinc(fc tau) I0(beta sqrt(1 - (tau / (P / 2))^2)) / I0(beta)
 *   each phase divided by its own float64 sum (DC gain 1), each coefficient then rounded once to fp32.  o, n >= 1, P even and in
 *   [4, 256], n * P <= 2^20, beta finite and >= 0; anything else: P2PHD_EINVAL.
 * p2phd_rateconv_out_len (host): L_out = ceil(frames * n / o) for 0 <= frames <= 2^40; -1 with an error text otherwise.
 * p2phd_rateconv_fwd: planar [channels][ld] f32 rows of `frames` = L samples (layout and argument checks of p2phd_truepeak; rows may
 *   start at any float), table_dev: n * P f32 on the device, phase-major -- the caller's table, of any content.  out: [channels][out_ld]
 *   f32 rows of out_frames = L_out samples, which must not overlap the input.  x~ is the row, 0 outside [0, L); a NaN or infinite
 *   sample is a sample like any other.  Output m = j n + p with p = m mod n:
 *     y[m] = sum_{k = 0}^{P - 1} c[p][k] x~[j o + (p o) div n + k - half],   m = 0 .. L_out - 1
 *   as ONE fp32 accumulator that starts at +0 and takes acc = fma(c[p][k], x~, acc) for k ascending (one rounding per tap), so a y
 *   has one bit pattern whatever the grid, the tile and the number of rows.  Every output is written by one thread: no atomics, no
 *   workspace, nothing zeroed before the launch, no ordering rule between calls.  frames = 0: nothing is launched or written.  o and n
 *   must differ and share no divisor; a bad o, n or P, out_frames != L_out, a pitch shorter than its row, a null or misaligned
 *   pointer, an output that overlaps the input: P2PHD_EINVAL.
 * p2phd_rateconv_tile_len (host): input samples of a row that one workgroup's run of blocks covers for this (o, n, P) (tests place
 *   their lengths around its multiples); -1 for a bad shape.
 * ---------------------------------------------------------------------------------------- */
int p2phd_rateconv_plan(int in_rate, int out_rate, double passband, double atten_db, int* o, int* n, int* taps_per_phase, double* beta);
int p2phd_rateconv_taps_fill(int o, int n, int taps_per_phase, double beta, double cutoff, float* out);
int64_t p2phd_rateconv_out_len(int64_t frames, int in_rate, int out_rate);
int p2phd_rateconv_fwd(const float* planar, int64_t frames, int channels, int64_t ld, const float* table_dev, int o, int n, int taps_per_phase,
                       float* out, int64_t out_frames, int64_t out_ld, void* stream);
int64_t p2phd_rateconv_tile_len(int o, int n, int taps_per_phase);

/* ------------------------------------------------------------------------------------------
 * Noise-shaped dither of whole-file generation's output stage (--dither shaped), csrc/shaper.hip: an error-feedback quantiser in
 * front of the 16-bit rounding, PCM16 only.  Launch family "shaper" (a p2phd_pcm_encode_shaped with frames > 0 counts 1).  The
 * noise transfer function is 1 - sum_k h[k] z^-k: the quantisation noise leaves the band the ear hears best and gathers near the
 * Nyquist frequency.  p2phd_pcm_encode_ex and its TPDF dither are unchanged.
 *
 * The recursion runs along time and rounds, so it is parallel by definition and not by approximation: a chunk length L = `chunk` (a
 * multiple of 64 in [256, 2^20]) is part of what is computed.  The error history is zero at the start of every chunk: for channel c
 * of C = `channels` and sample n of the chunk that starts at j L, e[m] = 0 for m < j L, and
 *     y = x[c][n] * gain[0]              `gain`: device pointer read by the kernel, as in p2phd_pcm_encode_ex; NULL: y = x
 *     v = y * 32768                      exact
 *     u = v;  for k = K, K - 1, .., 1:  u = fmaf(-h[k], e[n - k], u)          one fmaf per tap, in this order: the newest error last
 *     d = the TPDF dither of p2phd_pcm_encode_ex for (seed, i = first_index + n * channels + c)
 *     w = u + d;  r = rintf(w)
 *     stored = r clamped to [-32768, 32767];  w NaN -> 0                      what p2phd_pcm_encode_ex stores for w
 *     e[n] = r - u  where w is finite, else 0                                 from the UNclamped r: |e| <= 1.5, no wind-up while clipping
 *   A chunk at least as long as the row is the plain sequential recursion.  Consequences: K = 0, or every h[k] = 0, gives the bytes of
 *   p2phd_pcm_encode_ex(dither = 1) on the same operands at any chunk length; a payload encoded in pieces has the bytes of one call if
 *   and only if every piece starts on a chunk boundary, and a first_index that is not a multiple of chunk * channels is refused; a
 *   sample's bits depend on the operands of its chunk alone, so runs, streams and grids repeat them.
 * p2phd_pcm_encode_shaped: planar f32 rows in, interleaved little-endian int16 out, laid out and checked as for p2phd_pcm_encode_ex
 *   (rows may start at any float, the payload at any byte).  `taps`: h[1..K] as K floats on the HOST (0 <= K <= 16; they travel as
 *   kernel arguments; NULL with K = 0), finite.  frames = 0: nothing is launched or written.  K outside [0, 16], a bad chunk or
 *   first_index, channels < 1, ld < frames, a null or misaligned pointer: P2PHD_EINVAL.  No workspace, no atomics, nothing zeroed
 *   before the launch, no ordering rule between calls.
 * p2phd_shaper_taps_fill (HOST only, no device, as p2phd_xover_taps_fill): the curve's h[1..K] into out (room for 16 floats) and K
 *   into *K -- float64 literals rounded once to fp32.  curve_id 0 "lipshitz9": 2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281,
 *   -0.569, 0.0847; 1 "e5": 2.033, -2.165, 1.959, -1.590, 0.6149; 2 "light3": 1.623, -0.982, 0.109 -- the 9-, 5- and 3-tap curves of
 *   Lipshitz, Vanderkooy and Wannamaker (1991) for 44.1 kHz as commonly carried; written from memory, their provenance could not be
 *   checked against a source, their behaviour under the recursion above is measured.
 * p2phd_shaper_tile_len (host): samples of the time tile a workgroup stages at once (tests place their lengths around it); -1 for
 *   channels outside [1, 65535] or a bad chunk.
 * ---------------------------------------------------------------------------------------- */
int p2phd_pcm_encode_shaped(const float* planar, int64_t frames, int channels, int64_t ld, const float* gain, const float* taps, int K,
                            int64_t chunk, uint64_t seed, int64_t first_index, void* out, void* stream);
int p2phd_shaper_taps_fill(int curve_id, float* out, int* K);
int64_t p2phd_shaper_tile_len(int channels, int64_t chunk);

/* ------------------------------------------------------------------------------------------
 * FLAC input, csrc/flac.hip: native FLAC streams (RFC 9639) for the feeder (host decoder) and for whole-file generation (device
 * decoder).  Launch family "flac" (a p2phd_flac_decode with nframes > 0 counts 2: the frame kernel and the element-wise kernel).
 *
 * The subset: the "fLaC" marker, optionally behind an ID3v2 tag (skipped); any metadata blocks (STREAMINFO is read, SEEKTABLE is
 * counted, the rest are skipped by length); 1 to 8 channels in all four channel assignments (independent, left/side, side/right,
 * mid/side); 8, 12, 16, 20 and 24 bits per sample; fixed and variable block size with every block-size and sample-rate code and coded
 * numbers of 1 to 7 bytes; CONSTANT, VERBATIM, FIXED (order 0 to 4) and LPC (order 1 to 32, precision 1 to 15, shift >= 0) subframes;
 * wasted bits; Rice residuals with 4- and 5-bit parameters, partition orders 0 to 15 and escape partitions (raw width 0 included); a
 * shorter last frame.  Refused with an error text: 32-bit samples, Ogg FLAC, a negative LPC shift, reserved codes, a sample rate,
 * channel count or sample size that changes mid-stream.
 *
 * A frame table has one row of P2PHD_FLAC_ROW_WORDS int64 per frame: byte offset into the file, byte length, first sample (as the
 * frame numbers it: frame number x the stream's block size, or the coded sample number), block size, channel assignment (0 .. 7:
 * that many + 1 independent channels, 8 left/side, 9 side/right, 10 mid/side), bits per sample.  Decoders place frame f of a table at
 * column first_sample[f] - first_sample[first frame decoded] of every output row.
 *
 * HOST only (no device, as p2phd_xover_taps_fill):
 * p2phd_flac_info: the stream's STREAMINFO and where its first frame starts.  total_samples = 0: not stated (p2phd_flac_index counts).
 * p2phd_flac_index: one row per frame into `table` (room for `cap` rows; cap = 0: the count alone) -> the number of frames, or -1
 *   with an error text that names the frame's number and byte offset.  Verifies every header's CRC-8 and every frame's CRC-16, that
 *   the frames chain without a gap from the first frame to the end of the file, that frame / sample numbers are consecutive, that
 *   rate, channels and sample size are STREAMINFO's in every frame, and, where STREAMINFO states a total, that the frames hold it.
 *   A frame ends at the first byte q behind its header where the CRC-16 of the frame's bytes so far closes and either the file ends
 *   or the header of the following frame (good CRC-8, the expected number) stands: bytes inside a frame that look like a header do
 *   not split it.  No sample is decoded.
 * p2phd_flac_decode_host: the reference decoder.  Frames [first_frame, first_frame + frame_count) of `table` -> out[c * ld + column],
 *   int32, the `channels` rows of the stream (decorrelation undone, wasted bits restored); a row whose assignment is not one of
 *   `channels` channels is P2PHD_EINVAL, as on the device: nothing is written beyond the rows the caller has.  Prediction sums are 64-bit throughout; every
 *   read is bounded by the frame's byte range of its table row: a frame whose bit stream runs past its end, or that holds a
 *   reserved code, is P2PHD_EINVAL with a text that names the frame -- never an overrun.
 * p2phd_flac_workspace_bytes: bytes of p2phd_flac_decode's workspace for `channels` rows of pitch `ld` (0: bad arguments).
 * p2phd_flac_tile_len, p2phd_flac_frames_per_workgroup: samples per step of the element-wise kernel's workgroup and frames per
 *   workgroup of the frame kernel (tests place their sizes around them).
 *
 * DEVICE:
 * p2phd_flac_decode: the file's bytes and `nframes` table rows on the device -> out[c * ld + column] = integer x 2^-(bits-1) as fp32
 *   (exact: the bits data/wavio.py's load returns for the same samples).  flac_frames_kernel: one lane per frame reads its frame in
 *   8-byte pieces, decodes every subframe (64-bit prediction sums; coefficients and a history of 32 samples in LDS) and leaves the
 *   integers in `workspace` (int32 [channels][ld]); flac_pcm_kernel: a workgroup per frame (at most 2^20 of them, each then walking several frames) undoes the decorrelation and scales.  A
 *   lane never reads outside [offset, offset + length) of its row nor beyond nbytes, and writes nothing for a row that does not fit
 *   (column + block size > ld).  A frame that runs out of bits or meets a reserved code is written as zeros in every channel and
 *   recorded in *status_dev by an integer atomicMin of (frame index << 8 | reason), reason one of P2PHD_FLAC_E_*: the CALLER sets
 *   *status_dev to P2PHD_FLAC_STATUS_NONE on the same stream in front of the call and reads it behind its own synchronisation.  A
 *   frame's samples depend on nothing but its bytes and its row: the same bits on every run, stream and grid.  nframes = 0: nothing
 *   is launched or written.  channels outside [1, 8], bits not one of the five, a null or misaligned pointer: P2PHD_EINVAL.
 * ---------------------------------------------------------------------------------------- */
#define P2PHD_FLAC_ROW_WORDS 6
#define P2PHD_FLAC_OK          0
#define P2PHD_FLAC_E_BITS      1   /* the bit stream runs past the frame's end */
#define P2PHD_FLAC_E_RESERVED  2   /* a reserved code, a negative LPC shift, non-zero padding */
#define P2PHD_FLAC_E_GEOMETRY  3   /* a partition or predictor order the block size does not allow */
#define P2PHD_FLAC_E_LENGTH    4   /* the subframes end short of the frame's length */
#define P2PHD_FLAC_E_ROW       5   /* a table row that does not fit the buffers, or whose assignment is not `channels` */
#define P2PHD_FLAC_STATUS_NONE 0xFFFFFFFFFFFFFFFFull
typedef struct p2phd_flac_streaminfo {
  int32_t sample_rate, channels, bits, min_block, max_block, seek_points;
  int64_t total_samples, first_frame_offset;
  uint8_t md5[16];
} p2phd_flac_streaminfo;
int p2phd_flac_info(const void* bytes, int64_t nbytes, p2phd_flac_streaminfo* info);
int64_t p2phd_flac_index(const void* bytes, int64_t nbytes, int64_t* table, int64_t cap);
int p2phd_flac_decode_host(const void* bytes, int64_t nbytes, const int64_t* table, int64_t first_frame, int64_t frame_count, int channels,
                           int32_t* out, int64_t ld);
size_t p2phd_flac_workspace_bytes(int channels, int64_t ld);
int p2phd_flac_tile_len(void);
int p2phd_flac_frames_per_workgroup(void);
int p2phd_flac_decode(const void* bytes_dev, int64_t nbytes, const int64_t* table_dev, int64_t nframes, int channels, int bits, float* out,
                      int64_t ld, void* workspace, uint64_t* status_dev, void* stream);
/* measurement only (tools/time_generate.py flac): p2phd_flac_decode's arguments and checks, launching the frame kernel alone (stage 1:
 * out is not written) or the element-wise kernel alone (stage 2: it reads whatever the workspace holds).  Counts 1. */
int p2phd_flac_decode_stage(int stage, const void* bytes_dev, int64_t nbytes, const int64_t* table_dev, int64_t nframes, int channels, int bits,
                            float* out, int64_t ld, void* workspace, uint64_t* status_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Coded WAV input, csrc/wavcodec.hip: RIFF/WAVE data chunks that hold G.711 mu-law (format tag 7), G.711 A-law (tag 6) or 4-bit
 * IMA/DVI ADPCM (tag 0x11) for the feeder (host decoders) and for whole-file generation (device decoders).  Launch family
 * "wavcodec" (a p2phd_g711_decode or p2phd_ima_decode with frames > 0 counts 1).  Integer arithmetic; a coded file decodes to exactly
 * the samples its PCM16 twin holds, and every sample is scaled as data/wavio.py scales 16-bit PCM: float32(int16) * (1 / 32768).
 * Restated in tests/_wavcodec_ref.py; MS ADPCM (tag 2), GSM 6.10, G.726 and MP3-in-WAV are not built (data/wavio.py refuses them).
 *
 * mu-law byte b:  u = ~b & 0xFF, e = (u >> 4) & 7, m = u & 15, mag = (((m << 3) + 0x84) << e) - 0x84;
 *                 sample = u & 0x80 ? -mag : mag                                                        (within +-32124)
 * A-law byte b:   a = b ^ 0x55, e = (a >> 4) & 7, m = a & 15, mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
 *                 sample = a & 0x80 ? mag : -mag                                                        (within +-32256)
 * A G.711 payload is interleaved: byte n * C + c is frame n of channel c.
 *
 * IMA ADPCM, the block layout of a WAVE file: a block is `block_align` bytes.  Per channel it starts with a 4-byte header -- int16
 * little-endian predictor, uint8 step index, one ignored byte -- and the predictor is the block's first output sample of that
 * channel.  After the C headers come groups of 4 * C bytes: 4 bytes (8 nibbles) of channel 0, 4 of channel 1, ...; the low nibble of
 * a byte comes first.  Samples per block: spb = 1 + 8 * (block_align - 4 * C) / (4 * C), which needs block_align >= 8 * C and
 * (block_align - 4 * C) % (4 * C) == 0.  The step for nibble n with st = STEP[index]:
 *     d = (st >> 3) + (n & 1 ? st >> 2 : 0) + (n & 2 ? st >> 1 : 0) + (n & 4 ? st : 0)
 *     pred = clamp(n & 8 ? pred - d : pred + d, -32768, 32767);   index = clamp(index + {-1, -1, -1, -1, 2, 4, 6, 8}[n & 7], 0, 88)
 * with STEP the 89-entry table 7, 8, 9, ..., 32767.  A header's step index is clamped to 0 .. 88 where it is loaded, by every
 * decoder: no byte stream indexes past the table (p2phd_ima_scan_host is how a caller refuses such a file instead).
 * `nbytes` of payload hold p2phd_ima_frames(nbytes, ...) frames: spb per whole block, and 1 + 8 * k for a trailing partial block
 * that holds the C headers and k >= 0 whole groups; anything shorter is ignored.
 *
 * HOST only (no device, plain C++):
 * p2phd_g711_decode_host: `frames` frames of `channels` interleaved bytes -> out[c * ld + n] f32.  law: P2PHD_G711_ULAW / _ALAW.
 * p2phd_ima_frames: the frames `nbytes` hold (above); -1 with an error text for channels outside [1, 8] or a block_align the formula
 *   does not admit.
 * p2phd_ima_decode_host: frames [first_frame, first_frame + frame_count) of the payload -> out[c * ld + (n - first_frame)] f32.  Only
 *   the blocks that cover the window are read; the window must lie inside p2phd_ima_frames(nbytes, ...).
 * p2phd_ima_scan_host: walks the block headers of every block that holds a sample -> the first block one of whose step indices is
 *   above 88, -1 where there is none, -2 with an error text for bad arguments.
 * p2phd_ima_blocks_per_workgroup, p2phd_ima_max_workgroups: the blocks one workgroup of the device decoder stages per trip for a
 *   layout (0: bad arguments), and the cap of its grid; more blocks than their product are walked with the grid's stride (tests
 *   place their sizes around them).  p2phd_g711_max_workgroups: the cap of the G.711 decoder's grid, 256 lanes of one 16-byte piece
 *   each per workgroup and trip.
 *
 * DEVICE (both decode through the routine the host entries call):
 * p2phd_g711_decode: payload on the device at any byte offset -> out[c * ld + n] f32, n < frames; nothing else of a row is written.
 *   Element-wise; a lane reads 16 bytes at once from the payload's first 16-byte boundary on.
 * p2phd_ima_decode: `nbytes` of payload on the device at any byte offset -> the first `frames` frames (frames at most
 *   p2phd_ima_frames(nbytes, ...): a `fact` chunk may cut inside a block) as out[c * ld + n] f32.  One launch: a workgroup stages
 *   its blocks' bytes into LDS with coalesced reads, one lane runs one (block, channel) chain from LDS and stores each group's 8
 *   samples as two 16-byte stores where they are aligned and all inside `frames`, one by one otherwise.  No atomics, no scratch.
 *   The same bits on every run, stream and grid.  A block_align above 65024 is P2PHD_EINVAL here (the host entries take it): a
 *   block then does not fit the 64 KiB of LDS beside the step table.
 * frames = 0: nothing is launched or written.  channels outside [1, 8] (G.711: [1, 65535], as p2phd_pcm_decode), an unknown law, a
 * block_align the formula does not admit, ld < frames, frames beyond the payload, a null or misaligned pointer: P2PHD_EINVAL.
 * ---------------------------------------------------------------------------------------- */
#define P2PHD_G711_ULAW 0   /* format tag 7 */
#define P2PHD_G711_ALAW 1   /* format tag 6 */
int p2phd_g711_decode_host(const void* bytes, int64_t frames, int channels, int law, float* out, int64_t ld);
int64_t p2phd_ima_frames(int64_t nbytes, int channels, int block_align);
int p2phd_ima_decode_host(const void* bytes, int64_t nbytes, int channels, int block_align, int64_t first_frame, int64_t frame_count,
                          float* out, int64_t ld);
int64_t p2phd_ima_scan_host(const void* bytes, int64_t nbytes, int channels, int block_align);
int p2phd_ima_blocks_per_workgroup(int channels, int block_align);
int p2phd_ima_max_workgroups(void);
int p2phd_g711_max_workgroups(void);
int p2phd_g711_decode(const void* bytes, int64_t frames, int channels, int law, float* out, int64_t ld, void* stream);
int p2phd_ima_decode(const void* bytes, int64_t nbytes, int channels, int block_align, int64_t frames, float* out, int64_t ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * FLAC output, csrc/flacenc.hip: the payload of the PCM encoder (pcm16 / pcm24) -> the frames of a native FLAC stream that decodes
 * to it byte for byte.  Launch family "flacenc" (a p2phd_flac_encode counts 3: the frame kernel, the scan of the frame lengths, the
 * gather).  Restated in tests/_flac_enc_ref.py.
 *
 * THE STREAM CONTRACT.  The stream is a function of (payload, channels, bits, L, rate, block) alone, to the byte: host encoder,
 * device encoder and restatement are compared with ==.  Every decision is taken on exact bit counts in 64-bit integers.
 *
 * Input: the interleaved little-endian payload, `bits` 16 or 24, `channels` C in 1..8, L >= 1 samples per channel, `rate` in
 *   1..1048575, `block` in 16..65535.
 * Framing: frames of `block` samples, the last one shorter (L - (frames - 1) * block); blocking-strategy bit 0, the frame number coded
 *   (1 to 6 bytes).  Block-size code: 1 for 192, 2..5 for 576 << i, 8..15 for 256 << i, else 6 (8-bit trailer) for a size <= 256, else 7
 *   (16-bit trailer).  Rate code: 1..11 for the rates of the table, else 13 (Hz in 16 bits) below 65536, else 14 (tens of Hz) where
 *   the rate divides by 10 and the quotient is below 65536, else 0 (from STREAMINFO).  Sample-size code 4 / 6.  CRC-8 (poly 0x07)
 *   closes the header, zero bits pad to the byte boundary, CRC-16 (poly 0x8005, init 0) closes the frame.
 * Per coded channel, bps = bits, + 1 for a side channel, bs = the frame's samples:
 *   CONSTANT (8 + bps bits) whenever all samples of the block are equal.
 *   VERBATIM: 8 + bs * bps bits.
 *   FIXED of order o in 0..4 with Rice partition order p in 0..min(8, trailing zeros of bs), a pair being admitted where
 *   (bs >> p) > o: 8 + o * bps + 2 + 4 + the sum over the 2^p partitions of (pbits + min over k of [n * (k + 1) + sum of (u >> k)]),
 *   u = (r << 1) ^ (r >> 31) the zig-zag of a residual r, n the partition's residuals (bs >> p, the first partition o fewer).
 *   bits 16: method 0, pbits 4, k in 0..14; bits 24: method 1, pbits 5, k in 0..30.  No escape partitions, no wasted bits, no LPC.
 *   Ties, a priority list: within a partition the smaller k; among the pairs (o, p) of equal bits the smaller p, and among those of
 *   equal p the smaller o -- so an equally cheap (1, 0) is taken before (0, 1).  FIXED is taken only where its bits are strictly
 *   fewer than VERBATIM's.
 * Stereo (C == 2): the best bits of L, R, M = (L + R) >> 1 and S = L - R are found as above; the assignment is the cheapest of
 *   independent (L + R), left/side (L + S), side/right (S + R), mid/side (M + S), ties in that order.  Any other C: independent.
 * File (written by the caller, data/flacio.py): "fLaC", one STREAMINFO with the last-block flag (min_block = max_block = block, the
 *   smallest and largest frame length, rate, channels, bits, total = L, MD5 of the payload or zeros), the frames.
 *
 * HOST only:
 * p2phd_flac_encode_plan: -> *nframes = ceil(L / block); *max_stream_bytes = the frames' worst case (16 header bytes, every subframe
 *   VERBATIM, the side channel's extra bit included, CRC-16: a true bound, FIXED being taken only where smaller);
 *   *workspace_bytes of p2phd_flac_encode.
 * p2phd_flac_encode_host: the reference encoder, one thread, no device: `stream` (room for cap >= max_stream_bytes) receives the
 *   frames back to back, lengths[f] each frame's bytes, lengths[nframes] their total.  It decides and counts with the routines the
 *   device encoder uses.
 * p2phd_flac_encode_threads, p2phd_flac_encode_scan_threads, p2phd_flac_encode_window_words: lanes of a frame's workgroup (samples
 *   per step of its writer), frames per step of the scan's one workgroup, and 32-bit words of the window of a frame's bit stream
 *   that the frame kernel keeps in LDS and stores when a step ends beyond it (tests place their sizes around all three).
 *
 * DEVICE:
 * p2phd_flac_encode: the same bytes and the same `lengths` from the payload on the device (any byte alignment), on `stream`.  One
 *   workgroup per frame; it reads nothing outside the payload's channels * L * bits / 8 bytes, writes exactly lengths[nframes] bytes
 *   of stream_dev and the nframes + 1 words of lengths_dev (8-byte aligned), and keeps each frame in a worst-case slot of `workspace`
 *   (8-byte aligned, workspace_bytes >= the plan's) until the gather.  Integer sums only, no float (with the LPC option below: float64 in the
 *   one routine of its steps 2 and 3, in one lane, from exact integers, in a written order), no atomics on global memory: the
 *   same bytes on every run and stream.  A cap or workspace below the plan's, arguments outside the ranges above, a null or
 *   misaligned pointer: P2PHD_EINVAL, nothing is launched.
 * ---------------------------------------------------------------------------------------- */
int p2phd_flac_encode_plan(int channels, int bits, int64_t L, int block, int64_t* nframes, int64_t* max_stream_bytes, int64_t* workspace_bytes);
int p2phd_flac_encode_threads(void);
int p2phd_flac_encode_scan_threads(void);
int p2phd_flac_encode_window_words(void);
int p2phd_flac_encode_host(const void* payload, int channels, int bits, int64_t L, int rate, int block, void* stream, int64_t cap, int64_t* lengths);
int p2phd_flac_encode(const void* payload_dev, int channels, int bits, int64_t L, int rate, int block, void* stream_dev, int64_t cap,
                      int64_t* lengths_dev, void* workspace, int64_t workspace_bytes, void* stream);
/* measurement only (tools/time_generate.py flacout): p2phd_flac_encode's arguments and checks, launching the frame kernel alone (stage 1:
 * the frames stay in the workspace's slots, stream_dev and lengths_dev are not written) or the frame kernel without its CRC-16, which
 * is then written as zeros (stage 2).  Counts 1. */
int p2phd_flac_encode_stage(int stage, const void* payload_dev, int channels, int bits, int64_t L, int rate, int block, void* stream_dev, int64_t cap,
                            int64_t* lengths_dev, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * FLAC output, LPC, csrc/flacenc.hip: an opt-in extension of the stream contract above.  The option is lpc_order M in 0..12 (12: the
 * largest order of FLAC's streamable subset up to 48 kHz).  With M = 0 the entries below give the bytes of p2phd_flac_encode_host /
 * p2phd_flac_encode, through the same kernels.  With M > 0 `block` is at most 16384 (the subset's largest block: a coded channel
 * as int32 is then 64 KiB); a larger one is refused.  Restated in tests/_flac_lpc_ref.py.
 *
 * THE STREAM CONTRACT for M > 0.  The stream is a function of (payload, channels, bits, L, rate, block, M) alone, to the byte: host
 * encoder, device encoder and restatement are compared with ==.  Per coded channel of a frame, samples x[0..bs), bps as above,
 * P = 13 bits of coefficient precision:
 * 1. Analysis signal, integers only.  a[n] = x[n] >> max(0, bps - 16) (arithmetic).  Welch window in integers: d = 2 n - (bs - 1),
 *    D = bs + 1, W[n] = ((D^2 - d^2) << 15) / D^2 (integer division).  v[n] = (a[n] W[n]) >> 15.  R[l] = sum over n = l .. bs - 1 of
 *    v[n] v[n - l] for l = 0 .. Mo, Mo = min(M, bs - 1).  |R| < 2^46: exact in int64 in any order of summation, and exact as a
 *    double.  R[0] = 0: no LPC candidate.
 * 2. Levinson-Durbin in float64 from double(R): IEEE add, multiply and divide only, in exactly this order, never contracted (the
 *    one __host__ __device__ routine both encoders call carries #pragma clang fp contract(off)).  err = R[0].  For i = 0 .. Mo - 1:
 *    acc = R[i + 1]; for j = 0 .. i - 1: acc = acc - lp[j] R[i - j].  k = acc / err.  new[j] = lp[j] - k lp[i - 1 - j] for j < i,
 *    new[i] = k.  err = err (1 - k k).  If err is not > 0 or not finite: stop, order i + 1 and all higher orders are not admitted.
 *    Otherwise lp = new is the predictor of order o = i + 1: x^[n] = sum over j of lp[j] x[n - 1 - j].
 * 3. Quantisation, float64, same rules.  cmax = max |lp[j]|; cmax = 0: the order is not admitted.  frexp(cmax) gives the exponent e;
 *    shift = P - 1 - e; shift < 0: not admitted; else shift = min(shift, 15).  Error feedback in index order: ee = ee + ldexp(lp[j],
 *    shift); q[j] = ee rounded half away from zero (floor(ee + 0.5) for ee >= 0, -floor(-ee + 0.5) otherwise), clamped to
 *    -2^12 .. 2^12 - 1; ee = ee - q[j].
 * 4. Residual.  r[n] = x[n] - ((sum over j < o of q[j] x[n - 1 - j]) >> shift) for n >= o, the sum in 64 bits, the shift arithmetic.
 *    An order is admitted only where every |r[n]| < 2^28 (an integer maximum: order-free), which keeps the widths of the Rice sums.
 *    Real payloads reach it (a low-passed block with full-scale alternation at its ends, which the window hides from the fit):
 *    tests/_flac_lpc_cases.py, bound_side.
 * 5. Cost of LPC (o, p), admitted where (bs >> p) > o, p in the range above: 8 + o bps + 4 + 5 + o P + 2 + 4 + the partitions' bits,
 *    exactly as FIXED counts them: the same k ranges, the same smaller-k tie rule.
 * 6. Choice.  The subframe is first chosen as above: CONSTANT, else VERBATIM, else FIXED.  An LPC pair replaces it only where its
 *    bits are strictly fewer; among LPC pairs of equal bits the smaller p, then the smaller o.  All orders 1 .. Mo are tried: no order
 *    estimate, no heuristic.  The stereo assignment is taken from the four best bit counts as above.
 * Written: subframe type 32 | (o - 1), the o warm-up samples, precision - 1 = 12 in 4 bits, the shift in 5, the o coefficients in 13
 *   bits each, then the residual as a FIXED subframe's.
 * Consequences: the predictor of order o does not depend on M, so a frame never grows with M, and p2phd_flac_encode_plan's worst case
 *   still bounds the stream and the workspace.
 * Float: the decisions stay exact integer bit counts.  Float64 appears in steps 2 and 3 alone; they run in one thread (host) or one
 *   lane (device), from exact integers, in the written order -- which is what makes their bits the same on both.
 *
 * HOST only:
 * p2phd_flac_lpc_analyse: steps 1 to 3 of one block: `samples` int32 [bs] (1 <= bs <= 16384, each fitting bps, bps 16 / 17 / 24 / 25),
 *   lpc_order M in 1..12 -> R int64 [13] (zeros above Mo); per order o = 1 .. 12, row o - 1: admitted[o - 1] (1 / 0: by steps 2 and
 *   3; the residual bound of step 4 is the encoders'), shift[o - 1], q int32 [12][12] (row o - 1: its o coefficients, zeros behind;
 *   all zeros where not admitted).
 * p2phd_flac_lpc_fit: steps 2 and 3 alone, through the routine both encoders call, from any R int64 [orders + 1] (orders in 0..12, each
 *   |R[l]| < 2^53) -> admitted, q, shift as above.  It exists so that the stop rule of step 2 can be held to the restatement: the
 *   autocorrelation of a windowed block is positive definite, and no block was found whose err ends <= 0 (a pure alternating +-A does
 *   not: the window keeps |k| below 1), so the tests feed it sequences R that no block produces.
 * p2phd_flac_encode_lpc_host: p2phd_flac_encode_host with the option.
 * DEVICE:
 * p2phd_flac_encode_lpc: p2phd_flac_encode with the option; the same plan, the same workspace, the same refusals, and still 3
 *   launches of the family "flacenc".  M > 0 runs the frame kernel's LPC instantiation: the workgroup keeps the coded channel's
 *   block as int32 and its analysis signal as int16 in dynamic LDS beside the state of the other instantiation (4 bytes a sample; the
 *   analysis signal in the LDS of the Rice sums where it fits, else 2 bytes a sample more: at most 139 920 bytes a workgroup), each lane sums its products v v into M + 1 int64 that are folded with LDS integer adds, lane 0 runs steps 2 and
 *   3, and every admitted order goes through the Rice sums and the partition fold of the FIXED orders with its residuals read from
 *   the image.  No atomics on global memory, no float outside lane 0's routine.
 * p2phd_flac_encode_lpc_stage: p2phd_flac_encode_stage with the option (measurement only, counts 1).
 * ---------------------------------------------------------------------------------------- */
int p2phd_flac_lpc_fit(const int64_t* R, int orders, int32_t* admitted, int32_t* q, int32_t* shift);
int p2phd_flac_lpc_analyse(const int32_t* samples, int bs, int bps, int lpc_order, int32_t* admitted, int32_t* q, int32_t* shift, int64_t* R);
int p2phd_flac_encode_lpc_host(const void* payload, int channels, int bits, int64_t L, int rate, int block, int lpc_order, void* stream, int64_t cap,
                               int64_t* lengths);
int p2phd_flac_encode_lpc(const void* payload_dev, int channels, int bits, int64_t L, int rate, int block, int lpc_order, void* stream_dev, int64_t cap,
                          int64_t* lengths_dev, void* workspace, int64_t workspace_bytes, void* stream);
int p2phd_flac_encode_lpc_stage(int stage, const void* payload_dev, int channels, int bits, int64_t L, int rate, int block, int lpc_order, void* stream_dev,
                                int64_t cap, int64_t* lengths_dev, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Activation tensors of the conv stack are NHWC ("channels last": [N, H, W, Cp]) with the channel
 * pitch Cp = p2phd_channel_pitch(C) = C rounded up to 8; pad channels hold zeros.  dtype is
 * P2PHD_F32 (exact-f32 MFMA, parity runs) or P2PHD_BF16 (bf16 MFMA, fp32 accumulate).
 * ---------------------------------------------------------------------------------------- */
int p2phd_channel_pitch(int channels);

#define P2PHD_ACT_NONE  0
#define P2PHD_ACT_LRELU 1   /* LeakyReLU(0.2), models/networks.py:342,350,358 */
#define P2PHD_ACT_TANH  2   /* models/networks.py:160,207 */
#define P2PHD_ACT_RELU  3

/* One Conv2d / ConvTranspose2d layer of models/networks.py.
 *   transposed = 0: nn.Conv2d(C, K, (R,S), stride, padding=pad); with pad_mode = 1 the layer is
 *                   nn.ReflectionPad2d(pad) followed by nn.Conv2d(..., padding=0) (networks.py:190,223-231);
 *   transposed = 1: nn.ConvTranspose2d(C, K, (R,S), stride, padding=pad, output_padding=opad) (:205).
 * Master weights keep the PyTorch layouts ([K,C,R,S], resp. [C,K,R,S]) in f32. */
typedef struct p2phd_conv_desc {
  int32_t N, C, H, W;
  int32_t K, R, S;
  int32_t stride, pad, pad_mode, transposed, opad;
  int32_t dtype;
  int32_t w_layout;   /* layout of the f32 master weights (and of dw): 0 = PyTorch ([K,C,R,S] / [C,K,R,S]), 1 = K-major [K][R][S][C] */
} p2phd_conv_desc;

/* K-major master weights (round 3): for plain stride-1 Conv2d layers without channel or K padding (the residual trunk, the
 * discriminator's 256 -> 512 layers: 95 % of the parameters) the packed forward row [tap][channel] IS the master row when the
 * optimiser keeps the weights as [K][R][S][C].  The forward pack is then a cast, the input-gradient pack a bf16 transpose per
 * tap, and the weight gradient lands with coalesced rows instead of through a re-ordering tile.  The Python mirror hands such
 * parameters to torch as permuted views of the flat buffer (state_dict and checkpoints are unchanged).
 * p2phd_conv_kmajor_ok: 1 if desc (w_layout ignored) may set w_layout = 1. */
int p2phd_conv_kmajor_ok(const p2phd_conv_desc* c);
int p2phd_conv_out_size(const p2phd_conv_desc* c, int* Ho, int* Wo);

/* Packed (K-contiguous, tap-major, zero-padded) weights for the forward (which = 0) or the input-gradient
 * (which = 1) launches; repack after every optimizer step. */
size_t p2phd_conv_packed_bytes(const p2phd_conv_desc* c, int which);
int p2phd_conv_pack_weights(const p2phd_conv_desc* c, int which, const float* w, void* packed, void* stream);
/* Variant id (>= 0; -1: bad descriptor) of the packed layout that the launches of (desc, which) read.  The layout depends on
 * more than the layer: a tap-skipping merged stride-2 launch orders the taps of half its sub-pixel classes differently, and
 * whether a launch skips depends on N, H, W and the "cls_skip" option.  A buffer packed for one desc serves another desc of
 * the same layer only if both report the same id -- a caller that caches packed weights keys the cache on it
 * (the reference runs inference on a smaller last batch between training steps: train.py:206 -> eval_model). */
int p2phd_conv_pack_layout(const p2phd_conv_desc* c, int which);

/* y = act(conv(x) + bias).  If stats != NULL (float [N][Cp_out][2], overwritten; act must be NONE) it receives, per
 * (n, channel), the MEAN and the SUM OF SQUARED DEVIATIONS from it of conv(x)+bias over the sample's plane -- what
 * InstanceNorm2d needs (networks.py:22).  Every wave of the conv epilogue stores the partial of its rows about its own
 * mean (plain stores into a table in `workspace`), a small kernel merges them in a fixed order (Chan et al.): no float
 * atomics (bit-reproducible) and no E[x^2] - E[x]^2 cancellation. */
/* scratch of the forward launch: the folded tensor of <= 4-channel layers and the per-wave statistics partials */
size_t p2phd_conv_fwd_workspace_bytes(const p2phd_conv_desc* c);
int p2phd_conv_fwd(const p2phd_conv_desc* c, const void* x, const void* packed_fwd, const float* bias, int act,
                   void* y, float* stats, void* workspace, void* stream);

/* fp8 forward of the wide stride-1 layers (BASELINE configs[4]: bf16 + fp8 MFMA conv weights; the reference analogue is its
 * AMP path, train.py:62-67,148-149).  Operands are OCP e4m3 on the block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 (unit e8m0 block scales: the layer's one
 * scale is applied in the epilogue; twice the bf16 MFMA rate), accumulation fp32, outputs bf16;
 * fp32 master weights, the bf16 activations and the whole backward pass are unchanged.
 *   p2phd_conv_fp8_eligible   : 1 if the layer can run this way (Conv2d, stride 1, C %% 16 == 0, R*S*C %% 128 == 0, desc.dtype BF16)
 *   p2phd_conv_fp8_pack_weights: per-layer scale = max|w| / 448 found on the device (no host sync), weights quantised into
 *                               `packed8` (p2phd_conv_fp8_packed_bytes); repack after every optimizer step
 *   p2phd_conv_fwd_fp8        : x8 = the e4m3 twin of the bf16 input written by p2phd_instnorm_act_fwd_q8 (scale 1);
 *                               y, stats, workspace as for p2phd_conv_fwd */
int p2phd_conv_fp8_eligible(const p2phd_conv_desc* c);
size_t p2phd_conv_fp8_packed_bytes(const p2phd_conv_desc* c);
int p2phd_conv_fp8_pack_weights(const p2phd_conv_desc* c, const float* w, void* packed8, void* stream);
int p2phd_conv_fwd_fp8(const p2phd_conv_desc* c, const void* x8, const void* packed8, const float* bias, int act,
                       void* y, float* stats, void* workspace, void* stream);

/* dx = conv^T(dy) (+ addend, same layout as dx).  Replaces autograd of F.conv2d / F.conv_transpose2d and, for
 * pad_mode = 1, of ReflectionPad2d as well (needs p2phd_conv_dgrad_workspace_bytes of scratch). */
size_t p2phd_conv_dgrad_workspace_bytes(const p2phd_conv_desc* c);
int p2phd_conv_dgrad(const p2phd_conv_desc* c, const void* dy, const void* packed_dgrad, const void* addend, void* dx,
                     void* workspace, void* stream);

/* Input gradient with the FIRST pass of the producer's InstanceNorm backward fused into its store loop (round 2).  dx is
 * the gradient of the tensor this conv read, which a previous layer produced as act(InstanceNorm(prev_y)); prev_y
 * [N,H,W,Cp(C)] are that layer's pre-normalisation values, prev_stats [N,Cp(C),2] its (mean, M2) statistics, prev_act its
 * activation (NONE / RELU / LRELU).  Besides dx (+ addend) the call leaves bstats [N,Cp(C),2] = per (n, c)
 * (sum g', sum g' * yhat), g' = dx * act'(yhat) -- exactly what p2phd_instnorm_act_bwd's reduce pass computes from (dx,
 * prev_y) in two more tensor reads -- summed in a fixed order (no atomics).  Feed it to p2phd_instnorm_act_bwd_apply.
 * Available when p2phd_conv_dgrad_bsum_ok(desc) (one direct gather-GEMM launch: no reflect padding, no W-fold, not the
 * dedicated 7x7 kernel); workspace: p2phd_conv_dgrad_bsum_workspace_bytes (this call does not need the plain dgrad workspace). */
int p2phd_conv_dgrad_bsum_ok(const p2phd_conv_desc* c);
/* advisory: 0 where the fused form is available but slower than p2phd_conv_dgrad + the two-pass backward (the plain input
 * gradient would run on the 256 x 256 tile, which has no fused store loop: the discriminator's 256 -> 512 layer) */
int p2phd_conv_dgrad_bsum_pays(const p2phd_conv_desc* c);
size_t p2phd_conv_dgrad_bsum_workspace_bytes(const p2phd_conv_desc* c);
int p2phd_conv_dgrad_bsum(const p2phd_conv_desc* c, const void* dy, const void* packed, const void* addend, void* dx,
                          const void* prev_y, const float* prev_stats, int prev_act, float eps, float* bstats,
                          void* workspace, void* stream);
/* The same store loop for a producer WITHOUT InstanceNorm (Conv + ReLU / LeakyReLU(0.2)): x_act is that block's output --
 * the tensor this conv read -- and dx leaves multiplied by act'(x_act), i.e. as the gradient of the producer's
 * pre-activation; its activation-backward pass (p2phd_act_bwd / p2phd_act_bwd_db) is then not needed.  Same availability
 * and workspace as p2phd_conv_dgrad_bsum. */
int p2phd_conv_dgrad_act(const p2phd_conv_desc* c, const void* dy, const void* packed, const void* addend, void* dx,
                         const void* x_act, int prev_act, void* workspace, void* stream);

/* Which gather-GEMM tile would each generic launch of (desc, form) take under the current options?  Host arithmetic only:
 * nothing is launched and no device is needed (tests pin the answers and compare them with p2phd_launch_count).
 *   form : 0 forward | 1 input gradient on its generic plans | 2 input gradient on the exact reflect grid, dy expanded |
 *          3 the same through the reflection extras (p2phd_conv_dgrad_rx) | 4 fp8 forward
 *   flags: 1 InstanceNorm statistics wanted (forms 0, 4) | 2 fused InstanceNorm-backward sums (p2phd_conv_dgrad_bsum) |
 *          4 fused activation backward (p2phd_conv_dgrad_act); 2 and 4 belong to form 1, one at a time
 * Writes 9 ints per launch, for up to `cap` launches: tile rows, tile columns, 32-row blocks per wave, 32-column blocks per
 * wave, LDS ring slots, HALO loop (0 | 1), M tiles across samples (0 | 1), tap-skipping merged launch (0 | 1), and the rows per
 * statistics slot / fused-sums partial.  Returns the number of launches, or a negative error code when the form or a flag does
 * not apply to the layer.  A dedicated kernel may serve the layer instead: the answer is what the generic path would run. */
int p2phd_conv_gconv_tiles(const p2phd_conv_desc* c, int form, int flags, int* out9, int cap);

/* dw (master layout, f32, overwritten) and db (f32 [K], overwritten, may be NULL) from x and dy. */
size_t p2phd_conv_wgrad_workspace_bytes(const p2phd_conv_desc* c);
int p2phd_conv_wgrad(const p2phd_conv_desc* c, const void* x, const void* dy, float* dw, float* db, void* workspace,
                     void* stream);
/* Same, but dw += and db += : the gradient lands straight in the optimiser's (zeroed) flat gradient buffer, which
 * replaces one temporary and one `grad += new` launch per parameter of autograd's AccumulateGrad. */
int p2phd_conv_wgrad_acc(const p2phd_conv_desc* c, const void* x, const void* dy, float* dw, float* db, void* workspace,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * HBM-bound companions (csrc/norm.hip).  NHWC tensors, channel pitch = p2phd_channel_pitch(C).
 * ---------------------------------------------------------------------------------------- */

/* out = act((y - mean) * rstd) + residual: InstanceNorm2d(affine=False, eps) (networks.py:22) + ReLU /
 * LeakyReLU(0.2) / none, + the ResnetBlock skip (networks.py:252) or the LocalEnhancer sum (:180) when
 * residual != NULL.  stats = the float [N][Cp][2] (mean, sum of squared deviations) p2phd_conv_fwd wrote. */
int p2phd_instnorm_act_fwd(int dtype, const void* y, const float* stats, const void* residual, void* out,
                           int N, int64_t HW, int C, float eps, int act, void* stream);
/* Same, and additionally out8 = out as OCP e4m3 bytes (scale 1, saturated at +-448; dtype must be BF16): the operand of
 * the next layer's p2phd_conv_fwd_fp8. */
int p2phd_instnorm_act_fwd_q8(int dtype, const void* y, const float* stats, const void* residual, void* out, void* out8,
                              int N, int64_t HW, int C, float eps, int act, void* stream);
/* dy from g = dL/d(out) through act and InstanceNorm; bstats: float [N][Cp][2] scratch (zeroed inside).
 * db (float [C], may be NULL): the conv bias gradient = column sums of dy, accumulated in the same pass. */
int p2phd_instnorm_act_bwd(int dtype, const void* g, const void* y, const float* stats, float* bstats, void* dy,
                           float* db, int N, int64_t HW, int C, float eps, int act, void* stream);
/* Same, with db += instead of db = (see p2phd_conv_wgrad_acc). */
int p2phd_instnorm_act_bwd_acc(int dtype, const void* g, const void* y, const float* stats, float* bstats, void* dy,
                               float* db, int N, int64_t HW, int C, float eps, int act, void* stream);
/* The second (apply) pass alone, with the sums already in bstats (p2phd_conv_dgrad_bsum); db_accumulate != 0 adds the bias
 * gradient into db instead of overwriting it.  Only for planes that take the two-pass form:
 * p2phd_instnorm_act_bwd_two_pass(dtype, N, HW, C) != 0 (small planes use a single register-resident launch). */
int p2phd_instnorm_act_bwd_two_pass(int dtype, int N, int64_t HW, int C);
/* Host query (no launch, no stream, no device call): the grid of a reduction launch whose partial rows live in the library's
 * reduction scratch (see "Streams").  family "instnorm_bwd": the two-pass p2phd_instnorm_act_bwd / _acc on N samples of P pixels;
 * family "act_bwd_db": p2phd_act_bwd_db on P pixels (N must be 1).  *rows_wanted = workgroups per sample the plane would take
 * without the scratch limit, *rows_used = workgroups per sample of the launch that writes the partial rows: rows_used < rows_wanted
 * says that the launch is clamped to its region (then the InstanceNorm apply pass still runs on rows_wanted), and
 * rows_used * 256 is a multiple of the pieces per pixel (Cp / 8 in 16-bit storage, Cp / 4 in f32).  Both 0: nothing to launch, or
 * an InstanceNorm plane that takes the single launch.  The launchers take their grids from the same function, and where they
 * refuse (more samples than tickets, a region too small for one grid unit of rows, more channels than the backward kernels hold)
 * the query returns P2PHD_EINVAL with their error text; an unknown family is P2PHD_EINVAL too. */
int p2phd_reduction_rows(const char* family, int dtype, int N, int64_t P, int C, int* rows_wanted, int* rows_used);
/* Host query (no launch, no stream, no device call): the grid of a grid-stride kernel -- min(cdiv(work items, 256), cap)
 * workgroups of 256 threads, the work beyond walked with the grid's stride.  *wanted = workgroups (per row) without the cap,
 * *used = workgroups launched: used < wanted says that the kernel loops.  *unit_work = how much of `work` one trip of the whole
 * grid covers (work > 2 * unit_work: some thread takes a third trip).  The launchers take their grids from the same function.
 * `work` per family, and the cap:
 *   segments_gather(_planar), segments_stitch(_planar)   outputs per row (S * T, resp. L_out); a quad per thread; 16384
 *   segments_gather_ragged, segments_stitch_ragged       outputs of the longest clip row (S_j * T, resp. L_j); a quad per thread;
 *                                                         1024 per clip row (grid.y = clip rows, up to 65535 of them)
 *   segments_stitch_stream                                outputs per channel of the window (n_out); a quad per thread; 1024 per
 *                                                         channel (grid.y = channels)
 *   pcm_decode(_ex), pcm_encode, pcm_encode_ex            interleaved samples (frames * channels); 16384
 *   pcm_peak                                              frames per row, rows = channels; four 16-byte pieces in flight per
 *                                                         thread; min(2048 / channels, what the reduction scratch holds)
 *   stereo_matrix / stereo_matrix_scalar                  samples per row L, on the 16-byte path / the path of any alignment; 4096
 *   loudness_blocks, loudness_short_term                  blocks (J - 3, resp. J - 29); 2048
 *   avgpool3s2_fwd, avgpool3s2_bwd, nhwc_to_nchw, nchw_cat_to_nhwc   16-byte pieces of the NHWC side (N * pixels * Cp / 8 in
 *                                                         16-bit storage, / 4 in f32: the pooled side forward); 8192
 *   nchw_to_nhwc                                          elements N * C * HW; 8192
 *   act_bwd                                               elements (a 16-byte piece per thread: dtype); 8192
 *   loss_fwd / loss_bwd                                   padded elements P * Cp; the grid is sized by pieces of 8 elements and a
 *                                                         thread has four 16-byte pieces in flight (dtype); 1024 / 2048
 *   adam_step, adam_step_dev, adam_step_scaled            floats, a float4 per thread; 4096
 *   grads_nonfinite  (inside adam_step_scaled)            floats, four float4 in flight per thread; 2048
 *   timed_pack_pair                                       pixels, a quad per thread; 16384
 *   spectro_encode, spectro_encode_ex                     elements channels * B * M * F of the normalisation pass; 8192
 *   spectro_stats  (inside spectro_encode(_ex))           elements of the noise rows; 1024
 *   spectro_range, range_fold / .._scalar                 floats, on the 16-byte path / the path of any alignment; 1024
 *   spectro_rows  (inside spectro_encode_rows)            floats F * M of one row, a float4 per thread: workgroups per row; 32
 * rows is looked at by pcm_peak only, dtype (P2PHD_F32, P2PHD_BF16) where a thread's piece depends on it.  work = 0: all three 0.
 * An unknown family is P2PHD_EINVAL. */
int p2phd_stream_grid(const char* family, int dtype, int64_t work, int rows, int64_t* unit_work, int* wanted, int* used);
/* Residual trunk (networks.py:231-252: ReflectionPad2d(1) + Conv2d 3x3 + InstanceNorm): the input gradient of such a conv reads
 * dy plus the pair-sum rows / columns of the reflection's adjoint.  For planes that take the single-launch InstanceNorm backward
 * the kernel that WRITES dy appends them: allocate dy with p2phd_conv_reflect_extras_elems(desc) extra elements right behind its
 * N*H*W*Cp (0 = this layer / plane has no such form), hand the extras pointer (= dy + N*H*W*Cp) to p2phd_instnorm_act_bwd_rx
 * (the single-launch backward: no bstats), and take the input gradient with p2phd_conv_dgrad_rx -- no expansion pass, no workspace.
 * db / db_accumulate as in p2phd_instnorm_act_bwd_apply. */
size_t p2phd_conv_reflect_extras_elems(const p2phd_conv_desc* c);
int p2phd_instnorm_act_bwd_rx(int dtype, const void* g, const void* y, const float* stats, void* dy, float* db, int db_accumulate,
                              int N, int H, int W, int C, float eps, int act, void* reflect_extras, void* stream);
int p2phd_conv_dgrad_rx(const p2phd_conv_desc* c, const void* dy_with_extras, const void* packed_dgrad, const void* addend, void* dx,
                        void* stream);
int p2phd_instnorm_act_bwd_apply(int dtype, const void* g, const void* y, const float* stats, const float* bstats, void* dy,
                                 float* db, int db_accumulate, int N, int64_t HW, int C, float eps, int act, void* stream);
/* dx = g * act'(.) evaluated from the saved activation OUTPUT a (tanh, LeakyReLU, ReLU). */
int p2phd_act_bwd(int dtype, const void* g, const void* a, void* dx, int64_t n_elems, int act, void* stream);
/* Same over [n_pixels][Cp] tensors, plus db[c] (+)= sum over pixels of dx[., c]: the conv bias gradient of a layer with a
 * fused activation and no norm (networks.py:342-343), without a second read of dx. */
int p2phd_act_bwd_db(int dtype, const void* g, const void* a, void* dx, int64_t n_pixels, int C, int act, float* db,
                     int db_accumulate, void* stream);

/* nn.AvgPool2d(3, stride=2, padding=[1,1], count_include_pad=False) (networks.py:165,308). */
int p2phd_avgpool3s2_fwd(int dtype, const void* x, void* y, int N, int H, int W, int C, void* stream);
int p2phd_avgpool3s2_bwd(int dtype, const void* dy, void* dx, int N, int H, int W, int C, void* stream);

/* Module-boundary layout converters: f32 NCHW [N,C,HW] <-> channels [ch_off, ch_off+C) of NHWC [N,HW,Cp]. */
int p2phd_nchw_to_nhwc(int dtype, const float* src, void* dst, int N, int C, int64_t HW, int Cp, int ch_off, void* stream);
int p2phd_nhwc_to_nchw(int dtype, const void* src, float* dst, int N, int C, int64_t HW, int Cp, int ch_off, void* stream);
/* torch.cat((x0, x1, ...), dim=1) of up to four f32 NCHW tensors (pix2pixHD_model.py:56,307,360: the discriminator's
 * input) straight into NHWC [N,HW,Cp]: `srcs` / `chans` are HOST arrays of nsrc device pointers / channel counts; every
 * 16-byte piece of dst is written once, pad channels as zeros (no memset of dst, one launch). */
int p2phd_nchw_cat_to_nhwc(int dtype, const float* const* srcs, const int* chans, int nsrc, void* dst, int N, int64_t HW, int Cp,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Losses and optimiser (csrc/loss.hip).
 * kind 0: mean((a - target)^2)  -- GANLoss with use_lsgan (networks.py:68-110)
 * kind 1: mean(|a - b|)         -- criterionFeat = L1Loss (pix2pixHD_model.py:99,391-398)
 * a, b: [P][Cp] activations with C valid channels; *out += coeff * mean; the backward reads the upstream
 * gradient from device memory (*grad_out) so no host synchronisation is needed.
 * ---------------------------------------------------------------------------------------- */
int p2phd_loss_fwd(int kind, int dtype, const void* a, const void* b, float target, int64_t P, int C, float coeff,
                   float* out, void* stream);
int p2phd_loss_bwd(int kind, int dtype, const void* a, const void* b, float target, int64_t P, int C, float coeff,
                   const float* grad_out, void* da, void* stream);
/* torch.optim.Adam (no amsgrad / weight decay) over one flat f32 buffer; grads are scaled by grad_scale first
 * (1/world_size after a summing all-reduce).  step counts from 1. */
int p2phd_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                    float beta1, float beta2, float eps, int64_t step, float grad_scale, void* stream);
/* Same update with the learning rate and the step counter read from DEVICE memory (lr_dev: one float; step_dev: one
 * int64 holding the number of steps taken so far, incremented on the stream after the update): every launch argument
 * is then constant from step to step and the whole training step can be captured into a HIP graph and replayed. */
int p2phd_adam_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr_dev,
                        int64_t* step_dev, float beta1, float beta2, float eps, float grad_scale, void* stream);

/* Lazily normalised input (round 4; networks.py:190-195 and :205-207: the generator's outermost stride-2 layers at ngf 48, bf16).
 * p2phd_conv_lazy_ok(desc) = 1: this layer's forward and weight gradient can take `x_raw`, the PRE-normalisation output of the
 * InstanceNorm block in front of it, with that block's statistics [N][Cp][2] (mean, sum of squared deviations), activation and
 * eps, and apply (x - mean) * rstd + activation while staging rows -- the p2phd_instnorm_act_fwd pass over that plane is not run.
 * Results equal those computed from the materialised tensor, bit for bit.  Other arguments as p2phd_conv_fwd / p2phd_conv_wgrad
 * (`accumulate`: 0 = overwrite dw / db, 1 = add). */
int p2phd_conv_lazy_ok(const p2phd_conv_desc* c);
int p2phd_conv_fwd_lazy(const p2phd_conv_desc* c, const void* x_raw, const float* x_stats, int x_act, float x_eps,
                        const void* packed_fwd, const float* bias, void* y, float* stats, void* workspace, void* stream);
int p2phd_conv_wgrad_lazy(const p2phd_conv_desc* c, const void* x_raw, const float* x_stats, int x_act, float x_eps,
                          const void* dy, float* dw, float* db, int accumulate, void* workspace, void* stream);

/* Loss scaling for fp16 storage (torch.cuda.amp.GradScaler of train.py:62-67,165-181, device-resident so that a captured step
 * replays): scaler_state = 8 floats in device memory: [0] scale, [1] 1 / scale, [2] growth tracker, [3], [4] non-finite flags of
 * two gradient buffers (generator, discriminator).  The caller multiplies the loss by state[0] before its backward pass;
 * p2phd_adam_step_scaled = p2phd_adam_step_dev that first scans `grads` for inf / nan (flag 3 + found_index), unscales by
 * state[1] and SKIPS the update (and the step count) when the flag is set; p2phd_scaler_update = GradScaler.update(): backoff on
 * a flag, growth after growth_interval clean steps, flags cleared. */
int p2phd_adam_step_scaled(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr_dev,
                           int64_t* step_dev, float beta1, float beta2, float eps, float grad_scale, float* scaler_state,
                           int found_index, void* stream);
int p2phd_scaler_update(float* scaler_state, float growth_factor, float backoff_factor, int growth_interval, void* stream);

/* base[off, off + len) = 0 for n (off, len) pairs of int64 in DEVICE memory: one launch for the small segments of a flat
 * gradient buffer (the bias gradients, which several kernels add into; the weight gradients are overwritten by their first
 * writer of the step: p2phd_conv_wgrad vs p2phd_conv_wgrad_acc). */
int p2phd_zero_segments(float* base, const int64_t* seg_dev, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Spectrogram codec (csrc/spectro.hip): Pix2PixHDModel.to_spectro / denormalize / to_audio with
 * explicit_encoding (pix2pixHD_model.py:142-249).
 * encode: spec [B,F,M] f32 (MDCT4 output) -> log_spectro [B,2,M,F] in [0,1], pha [B,1,M,F],
 *   norm8 = (min, max, mean, std, noise_min, noise_max, -, -) on the device.  The top mask_rows bins are
 *   replaced by min-max scaled `noise` [B,2,mask_rows,F] (mask_mode 'mode2'), or zeros if noise == NULL.
 *   partials: scratch of p2phd_spectro_partials_floats(B,F,M) floats.
 * decode: log_spectro [B,2,M,F] + (min,max) -> spec [B,F,M] ready for IMDCT4.
 * ---------------------------------------------------------------------------------------- */
int64_t p2phd_spectro_partials_floats(int64_t B, int64_t F, int64_t M);
int p2phd_spectro_encode(const float* spec, int64_t B, int64_t F, int64_t M, float alpha, float min_value,
                         int mask_rows, const float* noise, float* log_spectro, float* pha, float* norm8,
                         float* partials, void* stream);
/* The general form (pix2pixHD_model.py:149-162,196-226).  channels = 2: explicit encoding as above; channels = 1:
 * log_spectro [B,1,M,F] = amplitude_to_DB(|spec| + min_value) min-max scaled, the sign in pha.  mask_mode 0 / 1 / 2 =
 * the reference's 'mode0' (noise / (max - min)), 'mode1' (min-max scaled noise times noise_sign, a +-1 tensor shaped
 * like noise) and 'mode2' (min-max scaled noise); noise == NULL = zeros (mask_mode None).  noise: [B,channels,mask_rows,F]. */
int p2phd_spectro_encode_ex(const float* spec, int64_t B, int64_t F, int64_t M, int channels, float alpha, float min_value,
                            int mask_rows, int mask_mode, const float* noise, const float* noise_sign, float* log_spectro,
                            float* pha, float* norm8, float* partials, void* stream);
int p2phd_spectro_decode(const float* log_spectro, const float* norm_min_max, int64_t B, int64_t F, int64_t M,
                         float alpha, float min_value, float* spec, void* stream);

/* util.imdct's decode (util/util.py:104-126; caller generate_audio.py:40-42): log_spectro [B,channels,M,F] (magnitudes are
 * taken), pha [B,M,F] (+-1), (min,max) -> signed amplitudes spec [B,F,M] * scale.  channels = 2 (explicit encoding):
 * amplitude = ch0 + ch1, sign = pha on rows < keep_rows and sign(ch0 - ch1) on the rest; channels = 1: sign = pha on every
 * row (the caller splices its random signs into pha, :122-123).  keep_rows = int(M * (1 / up_ratio)), or M. */
int p2phd_spectro_decode_signed(const float* log_spectro, const float* pha, const float* norm_min_max, int64_t B, int64_t F,
                                int64_t M, int channels, int keep_rows, float min_value, float scale, float* spec, void* stream);

/* The same decode (util/util.py:104-126) with the low band taken from the input: sr_log_spectro (the generator's) and
 * lr_log_spectro (the input's), both [B,channels,M,F] under the same (min,max).  With dec(X) = what
 * p2phd_spectro_decode_signed writes for X, row m of spec is
 *   dec(lr)[m]                                    m < keep_rows - fade_rows   (bit for bit)
 *   s + w (l - s), s = dec(sr)[m], l = dec(lr)[m]  keep_rows - fade_rows <= m < keep_rows,
 *       w = cos^2(pi (j + 1/2) / (2 fade_rows)), j = m - (keep_rows - fade_rows): the input's weight, fp32
 *   dec(sr)[m]                                    m >= keep_rows              (bit for bit)
 * A row reads only the tensors it decodes.  0 <= fade_rows <= keep_rows <= M.  One launch, nothing allocated, no
 * synchronisation: capturable. */
int p2phd_spectro_decode_spliced(const float* sr_log_spectro, const float* lr_log_spectro, const float* pha,
                                 const float* norm_min_max, int64_t B, int64_t F, int64_t M, int channels,
                                 int keep_rows, int fade_rows, float min_value, float scale, float* spec, void* stream);

/* One normalisation range for many encodes (whole-file generation, norm_scope='clip'): the range is found in a pass in front
 * of the encodes, accumulated on the device, and handed to each of them.
 * p2phd_spectro_range: the dB values p2phd_spectro_encode_ex computes for spec [B,F,M] (the same expressions in the same
 *   order; none is written), their minimum and maximum folded into the two floats at minmax_io on the device:
 *   minmax_io = (fminf(minmax_io[0], min), fmaxf(minmax_io[1], max)).  The caller starts it at (+inf, -inf); min and max do
 *   not depend on the order of the fold, so one call on a tensor leaves the norm8[0:2] p2phd_spectro_encode_ex leaves for it,
 *   bit for bit, and calls on the pieces of a tensor leave its range.  partials: p2phd_spectro_partials_floats(B,F,M) floats.
 * p2phd_range_fold: the same fold for n plain floats (the mask noise; NaN entries are passed over, as the encode's statistics
 *   pass them over).  partials: at least 4 * 1024 floats.
 * p2phd_spectro_encode_given: p2phd_spectro_encode_ex with the statistics read from norm8 on the device instead of computed
 *   -- [0], [1] the spectrum's min and max, [4], [5] the noise's (read only where noise rows are written), the layout that
 *   entry leaves -- and nothing written to norm8.  Under the tensor's own statistics it writes that entry's log_spectro and
 *   pha bit for bit, with one exception: a range of zero (max == min) gives the scale 0 where that entry divides by it, for
 *   the spectrum and for the noise alike, so digital silence under its own range encodes as zeros, not NaN.
 * Two launches (range, fold) or one (encode_given), none for B == 0 or n == 0; nothing allocated, no synchronisation, no
 * atomics: capturable.  Launch family "normscope", one per call that launches. */
int p2phd_spectro_range(const float* spec, int64_t B, int64_t F, int64_t M, int channels, float alpha, float min_value,
                        float* minmax_io, float* partials, void* stream);
int p2phd_range_fold(const float* x, int64_t n, float* minmax_io, float* partials, void* stream);
int p2phd_spectro_encode_given(const float* spec, int64_t B, int64_t F, int64_t M, int channels, float alpha, float min_value,
                               int mask_rows, int mask_mode, const float* noise, const float* noise_sign, const float* norm8,
                               float* log_spectro, float* pha, void* stream);

/* One normalisation range per row (whole-file generation, segment_norm): the rows of a batch no longer know of one another.
 * p2phd_spectro_encode_rows: p2phd_spectro_encode_ex applied to every row b of spec [B,F,M] on its own, in one call.  The
 *   statistics of row b go into norm_rows [B,8] (device, out) at 8 b + {0, 1, 4, 5}: the minimum and maximum of the row's dB values
 *   (p2phd_spectro_range's expressions, over all M bins and both channels) and of the row's [channels, mask_rows, F] noise
 *   ((+inf, -inf) without noise or with mask_rows == 0); the other four entries are 0.  NaN entries are passed over.  The row is
 *   then encoded as p2phd_spectro_encode_given encodes it under those eight floats: row b's log_spectro and pha are the bits
 *   p2phd_spectro_encode_ex writes for that row alone, except that a range of zero scales by 0 (spectrum and noise alike), so a
 *   row of digital silence encodes as zeros.  workspace: exactly p2phd_spectro_rows_partials_floats(B,F,M) floats (0 for a bad
 *   geometry), all written before they are read: no state is kept between calls.  The 16-byte read path is taken per row, by
 *   the alignment of that row's own base.  Three launches (statistics over a (chunk, row) grid, a fold per row, the encode).
 * p2phd_spectro_decode_signed_rows, p2phd_spectro_decode_spliced_rows: p2phd_spectro_decode_signed and
 *   p2phd_spectro_decode_spliced with the (min, max) of row b read at norm_rows[8 b], norm_rows[8 b + 1]; one launch each, the
 *   same kernels.
 * None launches for B == 0; B < 65536; nothing allocated, no synchronisation, no atomics: capturable.  Launch family
 * "normrows", one per call that launches. */
int64_t p2phd_spectro_rows_partials_floats(int64_t B, int64_t F, int64_t M);
int p2phd_spectro_encode_rows(const float* spec, int64_t B, int64_t F, int64_t M, int channels, float alpha, float min_value,
                              int mask_rows, int mask_mode, const float* noise, const float* noise_sign, float* norm_rows,
                              float* log_spectro, float* pha, float* workspace, void* stream);
int p2phd_spectro_decode_signed_rows(const float* log_spectro, const float* pha, const float* norm_rows, int64_t B, int64_t F,
                                     int64_t M, int channels, int keep_rows, float min_value, float scale, float* spec, void* stream);
int p2phd_spectro_decode_spliced_rows(const float* sr_log_spectro, const float* lr_log_spectro, const float* pha,
                                      const float* norm_rows, int64_t B, int64_t F, int64_t M, int channels, int keep_rows,
                                      int fade_rows, float min_value, float scale, float* spec, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation metrics (csrc/metrics.hip): compute_matrics (util/util.py:133-184).
 * hr, lr, sr [B,T] f32.  sr_matched [B,T] receives sr moment-matched to hr (:139-140); result4 (device) receives
 * (mse, snr_sr, snr_lr, lsd).  The LSD spectrogram is |STFT|^2 with n_fft2 = 2*opt.n_fft (power of two <= 4096),
 * hop2 = 2*opt.hop_length, window2 = kbdwin(2*opt.win_length) of win2 samples, reflect-centred when center != 0
 * (torchaudio.functional.spectrogram(pad=0, power=2, normalized=False) = torch.stft, :178-179).
 * tables: p2phd_stft_tables_floats(n_fft2) floats filled on the host; workspace: p2phd_metrics_workspace_bytes bytes.
 * ---------------------------------------------------------------------------------------- */
size_t p2phd_stft_tables_floats(int n_fft2);
int p2phd_stft_tables_fill(int n_fft2, float* host_out);
size_t p2phd_metrics_workspace_bytes(int64_t B, int64_t T, int n_fft2, int hop2, int win2, int center);
int p2phd_audio_metrics(const float* hr, const float* lr, const float* sr, int64_t B, int64_t T, int n_fft2, int hop2, int win2,
                        const float* window2, const float* tables, int center, float* sr_matched, float* result4,
                        void* workspace, void* stream);

/* The same figures per row, and the ones the reference's eval_matric.py leaves at zero.  Arguments as above; rows_out (device,
 * [B][8] f32) receives for every row b alone -- no mean over rows --
 *   mse, snr_sr, snr_lr, lsd, lsd_lf, lsd_hf, ssnr_sr, ssnr_lr;
 * matched_out [B][T] receives sr', the moment-matched sr; every sr figure is taken on sr', every lr figure on lr as given.
 *   lsd_lf / lsd_hf: per STFT frame sqrt(mean over the band's bins of (log10(P_hr + 1e-6) - log10(P_sr' + 1e-6))^2), averaged over
 *     the row's frames; the low band is k < cut_bin, the high band cut_bin <= k <= n_fft2/2 (lsd: all bins).  1 <= cut_bin <= n_fft2/2.
 *   ssnr_x: segmental SNR.  Frames of seg_win samples start at f * seg_hop, f < F = (T - seg_win) / seg_hop (integer division),
 *     window w[i] = 0.5 (1 - cos(2 pi (i + 1) / (seg_win + 1))); per frame 10 log10(Es / (En + eps) + eps) clamped to [-10, 35] with
 *     Es = sum (w hr)^2, En = sum (w hr - w x)^2, eps = 2^-52; the row's value is the mean over its F frames.  A row too short
 *     for one frame (F < 1) gets NaN in both slots; the call succeeds and the other six columns are valid.
 * Seven launches whatever B is, no host synchronisation, no atomics: a row's figures are the same bits from run to run and do
 * not depend on the other rows of the call.  workspace: p2phd_metrics_rows_workspace_bytes bytes (host arithmetic only; 0 and
 * p2phd_last_error() on bad arguments). */
size_t p2phd_metrics_rows_workspace_bytes(int64_t B, int64_t T, int n_fft2, int hop2, int win2, int center, int cut_bin,
                                          int seg_win, int seg_hop);
int p2phd_audio_metrics_rows(const float* hr, const float* lr, const float* sr, int64_t B, int64_t T, int n_fft2, int hop2, int win2,
                             const float* window2, const float* tables, int center, int cut_bin, int seg_win, int seg_hop,
                             float* matched_out, float* rows_out, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input feeder resampler (csrc/resample.hip): the HR -> LR -> HR conversions of data/audio_dataset.py:55-57,109-113
 * (torchaudio.functional.resample there; its source is not in the reference, so the definition -- Hann-windowed sinc,
 * lowpass_filter_width 6, rolloff 0.99 -- is this build's own, stated in oracle/feeder.py).
 * x [B,T] f32 -> out [B,T_out], T_out = p2phd_resample_out_len(T, orig, new) = ceil(new*T/orig).
 * kernel: p2phd_resample_kernel_floats floats, filled on the host by p2phd_resample_kernel_fill, then copied to the device.
 * ---------------------------------------------------------------------------------------- */
int p2phd_resample_geometry(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int* o, int* n, int* width,
                            int* klen);
size_t p2phd_resample_kernel_floats(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff);
int p2phd_resample_kernel_fill(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, float* host_out);
int64_t p2phd_resample_out_len(int64_t T, int orig_freq, int new_freq);
int p2phd_resample_fwd(const float* x, int64_t B, int64_t T, int orig_freq, int new_freq, int lowpass_filter_width,
                       double rolloff, const float* kernel, float* out, int64_t T_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* P2PHD_H */
