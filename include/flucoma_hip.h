/*
 * flucoma_hip.h -- C ABI of libflucoma_hip.so: the MI355X (gfx950) implementation of
 * flucoma-core's buffered spectral-decomposition hot path (STFT -> magnitude -> KL-NMF).
 *
 * This is the drop-in boundary.  Every entry point replaces a reference interface that is
 * cited next to it (paths relative to <flucoma-core>/include/flucoma/).  Plain pointers and
 * sizes only: no C++ types, no torch types, no exceptions cross this boundary.
 *
 * Conventions
 *   - status codes map 1:1 onto client::Result::Status (clients/common/Result.hpp:24);
 *     the message of the last non-OK result is read with fluhip_last_error().
 *   - "host" pointers are ordinary CPU memory; "dev" pointers are HIP device memory on the
 *     context's device.  Nothing is retained after a call returns except inside handles.
 *   - all matrices are dense row-major with the layouts of the reference's FluidTensorViews:
 *       spectrogram / magnitude  T x F       (F = fft/2 + 1, T = (N + hop) / hop)
 *       W1 (bases)               K x F
 *       H1 (activations)         T x K
 *   - the library is re-entrant; a context may be used by one thread at a time (the reference
 *     runs one job per std::thread: clients/common/FluidNRTClientWrapper.hpp:1048).
 *   - there is NO CPU fallback: without a usable gfx950 device every compute entry point
 *     returns FLUHIP_ERROR.
 */
#ifndef FLUCOMA_HIP_H
#define FLUCOMA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5 (round 6) = 4 + fluhip_last_error_is_out_of_memory, fluhip_clear_error (the host clients' batched -> channel-by-channel
 * fallback classifies by code: include/flucoma_hip/NMFClient.hpp needs them), fluhip_corpus_stft_mag_only,
 * fluhip_corpus_last_loop_ms, fluhip_debug_plan_shape, fluhip_debug_wnorm_form.  Nothing of version 4 changed meaning.
 * Added later within 5 (additive only): fluhip_nmfcross_process_f64, fluhip_griffinlim_f64, fluhip_bufnmfcross_f32,
 * fluhip_debug_cross_plan, fluhip_debug_jacobi_svd_f64, fluhip_novelty_curve_f64, fluhip_novelty_slices_f64,
 * fluhip_bufnoveltyslice_f32, fluhip_bufnoveltyfeature_f32, fluhip_debug_novelty_plan, fluhip_onset_curve_f64,
 * fluhip_onset_slices_f64, fluhip_bufonsetslice_f32, fluhip_bufonsetfeature_f32, fluhip_debug_onset_plan,
 * fluhip_debug_features_plan, fluhip_hpss_planes_f64, fluhip_bufhpss_f32, fluhip_debug_hpss_plan, fluhip_pitch_frames_f64,
 * fluhip_debug_pitch_curve_f64, fluhip_bufpitch_f32, fluhip_debug_pitch_plan, fluhip_debug_resynth_f64,
 * fluhip_debug_corpus_read_layouts_f64, fluhip_spectralshape_frames_f64, fluhip_bufspectralshape_f32,
 * fluhip_debug_chroma_filters_f64, fluhip_chroma_frames_f64, fluhip_bufchroma_f32, fluhip_debug_spectral_plan,
 * fluhip_loudness_frames_f64, fluhip_bufloudness_f32, fluhip_debug_loudness_plan, fluhip_amp_envelope_f64,
 * fluhip_amp_slices_f64, fluhip_bufampslice_f32, fluhip_bufampfeature_f32, fluhip_debug_amp_plan,
 * fluhip_debug_cross_stencil_f64, fluhip_amp_gate_f64, fluhip_bufampgate_f32, fluhip_debug_ampgate_plan,
 * fluhip_debug_stft_frames_f32, fluhip_debug_stft_frames_f64. */
#define FLUHIP_ABI_VERSION 5

/* clients/common/Result.hpp:24  enum class Status { kOk, kWarning, kError, kCancelled } */
enum fluhip_status
{
  FLUHIP_OK = 0,
  FLUHIP_WARNING = 1,
  FLUHIP_ERROR = 2,
  FLUHIP_CANCELLED = 3
};

/* algorithms/public/WindowFuncs.hpp:26-32  enum class WindowTypes */
enum fluhip_window
{
  FLUHIP_WINDOW_HANN = 0,
  FLUHIP_WINDOW_HANND = 1,
  FLUHIP_WINDOW_HAMMING = 2,
  FLUHIP_WINDOW_BLACKMANHARRIS = 3,
  FLUHIP_WINDOW_GAUSSIAN = 4
};

typedef struct fluhip_ctx    fluhip_ctx;    /* one device + one HIP stream + scratch arena */
typedef struct fluhip_corpus fluhip_corpus; /* a device-resident batch of equal-shape buffers */

/* algorithms/public/NMF.hpp:31 ProgressCallback = std::function<bool(index)>; invoked on the
 * calling thread with iteration = 1..iters in order; returning 0 cancels (NMF.hpp:175-176). */
typedef int (*fluhip_progress_fn)(int64_t iteration, void* user);

/* ---- library / context ------------------------------------------------------------- */
int         fluhip_abi_version(void);
int         fluhip_device_count(void);                    /* 0 when no HIP device is visible */
int         fluhip_ctx_create(int device, fluhip_ctx** out);
/* Teardown order: destroy every corpus created on a context BEFORE the context (a corpus keeps using its context's
 * stream until fluhip_corpus_destroy returns). */
void        fluhip_ctx_destroy(fluhip_ctx* ctx);
const char* fluhip_last_error(const fluhip_ctx* ctx);     /* never NULL */
/* 1 when the last non-OK result of this context was an allocation the device (hipErrorOutOfMemory, the FFT workspace) or
 * the host (std::bad_alloc inside the library) could not serve -- the one failure a caller may answer by retrying with a
 * smaller job (the clients' batched -> channel-by-channel fallback, NMFClient.hpp).  Classified by error CODE at the point
 * of failure, never by message text.  fluhip_clear_error empties message and flag (call it in front of a block of calls
 * whose failure you are going to classify, so that nothing stale is read). */
int         fluhip_last_error_is_out_of_memory(const fluhip_ctx* ctx);
void        fluhip_clear_error(fluhip_ctx* ctx);
/* device name / gcnArchName into caller buffers (for bench reports) */
int         fluhip_ctx_device_info(const fluhip_ctx* ctx, char* name, int name_len, char* arch,
                                   int arch_len, int* compute_units);
/* raw HIP stream (hipStream_t) the context launches on -- for event timing by the caller */
void*       fluhip_ctx_stream(const fluhip_ctx* ctx);
/* Device buffers are recycled through a per-device cache of freed blocks (at most 8 GiB per device; a context's
 * destruction empties its device's cache).  fluhip_ctx_trim hands the cached blocks of the context's device back to
 * the driver now -- for hosts that share the GPU with other allocators (torch, RCCL). */
int         fluhip_ctx_trim(fluhip_ctx* ctx);
int         fluhip_ctx_synchronize(fluhip_ctx* ctx);
/* How far the device may run ahead of the last iteration reported to a progress callback (default 8: at most 7 iterations
 * are enqueued beyond the one a callback refuses).  lag = 1 is the reference's exact behaviour -- NMF.hpp:175-176 stops AT the
 * iteration whose callback returns false, the factors are those of that iteration -- at the price of one host round trip per
 * iteration (~10 - 20 us: nothing for a corpus, a third of a single small buffer's iteration). */
int         fluhip_ctx_set_progress_lag(fluhip_ctx* ctx, int lag);

/* ---- parameter arithmetic (integer, bit-exact) --------------------------------------- */
/* clients/common/ParameterTypes.hpp:295-312 FFTParams::fftSize/hopSize/frameSize.
 * in: win, hop (<=0: win/2), fft (<0: nextPow2(win)).  Returns FLUHIP_ERROR when fft is not a
 * power of two >= win or win < 4 (the reference clamps these at set time: :371-393). */
int fluhip_fft_params(int64_t win, int64_t hop, int64_t fft, int64_t* win_out, int64_t* hop_out,
                      int64_t* fft_out, int64_t* bins_out);
/* algorithms/public/STFT.hpp:98-99, clients/nrt/NMFClient.hpp:111-112: (n + hop) / hop */
int64_t fluhip_stft_num_frames(int64_t n, int64_t win, int64_t hop);

/* ---- algorithm::STFT ------------------------------------------------------------------ */
/* Replaces STFT::STFT(win, fft, hop, windowType) + STFT::process(audio, spectrogram) +
 * STFT::magnitude(spectrogram, magnitude)  (algorithms/public/STFT.hpp:36-47, 90-108, 61-66).
 * audio: n host doubles with element stride `stride`.  spec (may be NULL): T*F interleaved
 * (re,im) doubles == std::complex<double>[T][F].  mag (may be NULL): T*F doubles, |spec| by hypot -- exact over the whole
 * double range, exactly 0 for a silent bin. */
int fluhip_stft_f64(fluhip_ctx* ctx, const double* audio, int64_t n, int64_t stride, int64_t win,
                    int64_t fft, int64_t hop, int window_type, double* spec, double* mag,
                    int64_t* frames_out);
/* same with the float->double conversion of clients/nrt/NMFClient.hpp:240 folded in */
int fluhip_stft_f32(fluhip_ctx* ctx, const float* audio, int64_t n, int64_t stride, int64_t win,
                    int64_t fft, int64_t hop, int window_type, double* spec, double* mag,
                    int64_t* frames_out);

/* Diagnostic: the inverse every resynthesising client runs (BufNMF, NMFFilter, BufHPSS, BufSTFT, Griffin-Lim), on the caller's
 * own doubles and with a double result -- RatioMask::process + ISTFT::process (algorithms/public/RatioMask.hpp:33-57,
 * STFT.hpp:178-199) through the same tables, kernels and choice of form (on-chip, or the global-memory passes above fft 8192).
 * spec: T x F interleaved (re,im) doubles; the imaginary parts of DC and Nyquist are ignored.  win, fft, hop as for the
 * forward transform; out sample i is position i + trim of the overlap-added frames (frame t at [t hop, t hop + win)) divided
 * by max(overlap-added window^2, eps): trim = win / 2 is ISTFT::process.  Positions no frame covers are 0.
 * W (K x F) and H (T x K), both NULL or both given: with them component k is the inverse of spec * min(H[t][k] W[k][f] *
 * (1 / max((H W)[t][f], eps)), 1), all K in one launch; out: max(K, 1) x n doubles (K is ignored without factors).
 * Bad arguments: FLUHIP_ERROR with a message that names them, out untouched. */
int fluhip_debug_resynth_f64(fluhip_ctx* ctx, const double* spec, int64_t T, int64_t win, int64_t fft, int64_t hop, int64_t n,
                             int64_t trim, const double* W, const double* H, int64_t K, double* out);

/* Diagnostic: T frames of each of B buffers from an arbitrary first sample -- frame t of a buffer is its samples
 * [frame0 + t hop, + win), zero outside [0, n); frame0 may lie any distance before the buffer and the frames may run any
 * distance behind it -- through the same tables, launch and choice of kernel form as every client's forward transform.
 * padded: B x (guard + n + guard) samples, every buffer's n samples between `guard` samples of the caller's choosing, which
 * no result may depend on; guard >= the furthest any frame lies outside its buffer + fft (checked), so that nothing a kernel
 * loads for these frames leaves the call's own allocation.  spec: B x T x F interleaved (re,im) doubles, mag: B x T x F
 * doubles, either may be NULL.  With spec the magnitudes are hypot of it, as fluhip_stft_* return them (exactly 0 for a silent
 * bin); without it they are the kernels' own, as the corpus and the control clients consume them (the block form leaves
 * sqrt(DBL_MIN) = 2^-511 for an exactly silent bin).  Bad arguments: FLUHIP_ERROR with a message that names them. */
int fluhip_debug_stft_frames_f32(fluhip_ctx* ctx, const float* padded, int64_t B, int64_t n, int64_t guard, int64_t win,
                                 int64_t fft, int64_t hop, int64_t frame0, int64_t T, double* spec, double* mag);
int fluhip_debug_stft_frames_f64(fluhip_ctx* ctx, const double* padded, int64_t B, int64_t n, int64_t guard, int64_t win,
                                 int64_t fft, int64_t hop, int64_t frame0, int64_t T, double* spec, double* mag);

/* ---- algorithm::NMF ------------------------------------------------------------------- */
/* Replaces NMF::process(X, W1, H1, V1, rank, nIterations, updateW, updateH, randomSeed, W0, H0)
 * + NMF::addProgressCallback  (algorithms/public/NMF.hpp:91-139, 144-183).
 * X: T x F with row stride ldx (doubles).  W0: K x F or NULL ("0x0 view").  H0: T x K or NULL.
 * W1: K x F, H1: T x K, V1: T x F or NULL.  seed < 0 => std::random_device like the reference.
 * progress is called once per completed iteration, in order; the device is never more than 8 iterations ahead of the last
 * one reported.  On cancellation returns FLUHIP_CANCELLED; W1/H1 then hold the factors as they stand when the device has
 * stopped -- at most 7 iterations after the one the callback refused (the reference stops at it exactly, NMF.hpp:175-176;
 * its client discards the factors of a cancelled job, clients/nrt/NMFClient.hpp:273-274) -- and V1 is left unwritten.
 * fluhip_ctx_set_progress_lag(ctx, 1) makes the stop exact.
 * Numerics: FP64 throughout.  The quotients V / max(W H, eps) of the update loop are formed as V * (1 / d) with a Newton-
 * refined reciprocal, relative error <= 2^-46 (1.4e-14) per quotient instead of a correctly rounded division; measured,
 * the factors stay within 1e-13 of the restatement after 200 iterations (the tests assert 1e-9; north_star asks 1e-5).
 * The reciprocals of four quotients (six in the frame-strip kernel) come from one reciprocal of their product, which stays
 * inside the double range while max|X| <= 2^128 (~3.4e38; any float input).  Larger X, up to DBL_MAX, is scaled by the
 * smallest power of two 2^-e that brings it to 2^128 and H1 / V1 are scaled back by 2^e (exact; W is scale-free); input at
 * or below 2^128 is not rescaled and keeps its arithmetic bit for bit.  The same holds for fluhip_nmf_process_frames_f64.
 * One deviation: past ~1e154 the reference's own W.colwise().normalize() overflows and it returns zeros, where this
 * library returns finite factors.  Build with -DFLUHIP_QUOTIENT_CORRECTION=1 for division to the last bit. */
int fluhip_nmf_process_f64(fluhip_ctx* ctx, const double* X, int64_t T, int64_t F, int64_t ldx,
                           int64_t K, int64_t iters, int update_w, int update_h, int64_t seed,
                           const double* W0, const double* H0, double* W1, double* H1,
                           double* V1, fluhip_progress_fn progress, void* user);

/* The same with every matrix as a two-stride view, the shape FluidTensorView<double, 2> hands to asEigen
 * (data/FluidTensor_Support.hpp:260-420 strides, :386-393 transpose(); util/FluidEigenMappings.hpp:35-225 maps them as
 * Stride<Dynamic, Dynamic>): element (r, c) at data[r * row_stride + c * col_stride].  NULL, data == NULL or a zero
 * extent is the reference's "0x0 view" (no seed / output not wanted).  Shapes as above (X T x F, W0 / W1 K x F,
 * H0 / H1 T x K, V1 T x F).  Unit-column-stride views and their transposes (unit row stride) move as strided copies
 * with no host-side repacking of X or V1; views with two non-unit strides are packed on the host. */
typedef struct fluhip_matrix_view
{
  double* data;
  int64_t rows, cols, row_stride, col_stride;
} fluhip_matrix_view;
int fluhip_nmf_process_views_f64(fluhip_ctx* ctx, const fluhip_matrix_view* X, int64_t K, int64_t iters, int update_w,
                                 int update_h, int64_t seed, const fluhip_matrix_view* W0, const fluhip_matrix_view* H0,
                                 const fluhip_matrix_view* W1, const fluhip_matrix_view* H1, const fluhip_matrix_view* V1,
                                 fluhip_progress_fn progress, void* user);

/* Replaces NMF::processFrame(x, W0, out, nIterations, v, randomSeed, alloc) (algorithms/public/NMF.hpp:45-89)
 * applied to every row of X at once -- the per-frame activation solve that
 * clients/rt/NMFMatchClient.hpp:113-118 (10 iterations, no estimate) and clients/rt/NMFFilterClient.hpp:102-116
 * (kIterations, estimate kept for the ratio mask) run on each spectral frame.  Frames are independent, so the
 * whole matrix is one batch of the H update with the dictionary fixed.
 * X: T x F magnitudes with row stride ldx.  W0: K x F dictionary (read only here; the reference clamps and
 * row-normalises its argument in place -- pass a copy there, the result is the same).
 * H (may be NULL): T x K activations.  V (may be NULL): T x F estimates W^T h.
 * seed >= 0: every frame starts from the same K draws, like the reference's fresh generator per call;
 * seed < 0: std::random_device. */
int fluhip_nmf_process_frames_f64(fluhip_ctx* ctx, const double* X, int64_t T, int64_t F, int64_t ldx,
                                  const double* W0, int64_t K, int64_t iters, int64_t seed, double* H, double* V);

/* ---- algorithm::NNDSVD / client::nndsvd::NMFSeedClient ------------------------------------------ */
/* Replaces NNDSVD::process(X, W, H, minRank, maxRank, amount, method, seed) (algorithms/public/NNDSVD.hpp:30-132):
 * thin SVD of X^T (bins x frames), rank k = the smallest number of leading singular values covering `amount`
 * of their sum (clamped to [min_rank, max_rank]; amount == 0 => min_rank), then the non-negative factors
 * method 0 (NMF-SVD): W = |U_k|, H = |S_k V_k^T|;  1 (NNDSVDar) / 2 (NNDSVDa) / 3 (NNDSVD): positive/negative
 * split of every singular pair, zeros filled with small random values / the mean / left at zero.
 * X: T x F with row stride ldx.  W: w_rows x F, H: T x w_rows (the reference's W.rows(); rows / columns >= k are
 * zero, or filled like the rest for methods 1 and 2, exactly as the reference treats its zero-initialised
 * outputs); k is returned in *rank_out and must not exceed w_rows.
 * The SVD is a one-sided Jacobi iteration on the device (kernels_svd.hip) on X scaled by a power of two to max|X| ~ 1 (as
 * Eigen's and LAPACK's SVDs scale), so any finite magnitude is handled.  A singular pair is only defined up to a
 * common sign:
 * method 0 does not depend on it, methods 1..3 do (in the reference as well -- they follow whatever Eigen's
 * BDCSVD returns), so for those only the construction from a given SVD is pinned by the tests. */
int fluhip_nndsvd_f64(fluhip_ctx* ctx, const double* X, int64_t T, int64_t F, int64_t ldx, int64_t w_rows,
                      int64_t min_rank, int64_t max_rank, double amount, int method, int64_t seed, double* W,
                      double* H, int64_t* rank_out);
/* Replaces NMFSeedClient::process (clients/nrt/NMFSeedClient.hpp:73-131; BufNMFSeed): STFT -> magnitude ->
 * NNDSVD -> bases (max_rank x F floats, rows >= rank untouched by the reference's resize-to-rank: here zero) and
 * activations (max_rank x T floats, scaled by 1 / max over the whole T x max_rank envelope matrix, :120-128).
 * Silence: the reference's 1 / max is 1 / 0 and every envelope it writes NaN; here, when acts_out is asked for,
 * FLUHIP_ERROR ("silent input ...").  With acts_out == NULL there is no 1 / max and silence gives its (finite) bases.
 * Likewise, in both entry points, where methods 1..3 meet an exactly zero singular pair within the rank asked for (0 / 0
 * in alg/NNDSVD.hpp:90-100): FLUHIP_ERROR instead of NaN factors.  On these errors neither entry point writes any of its
 * outputs (W, H, bases_out, acts_out, *rank_out keep what they held). */
int fluhip_bufnmfseed_f32(fluhip_ctx* ctx, const float* audio, int64_t n, int64_t stride, int64_t win,
                          int64_t fft, int64_t hop, int64_t min_rank, int64_t max_rank, double coverage,
                          int method, int64_t seed, float* bases_out, float* acts_out, int64_t* rank_out);

/* Diagnostic: the SVD the two entry points above run, whole.  X: T x F with row stride ldx (any sign).  With r = min(F, T):
 * s [r] descending, U [r x F] (row j = u_j), VT [r x T] with X^T = sum_j s_j u_j v_j^T, *sweeps_out (may be NULL) the
 * number of Jacobi sweeps taken (the iteration gives up with FLUHIP_ERROR after 40).  The same upload, transpose, scaling,
 * sweeps, sort and normalisation as fluhip_nndsvd_f64; the rows of VT that belong to an exactly zero s_j are zero. */
int fluhip_debug_jacobi_svd_f64(fluhip_ctx* ctx, const double* X, int64_t T, int64_t F, int64_t ldx, double* s,
                                double* U, double* VT, int64_t* sweeps_out);

/* ---- client::bufnmf::NMFClient::process, one channel ---------------------------------- */
/* Replaces the body of the channel loop, clients/nrt/NMFClient.hpp:240-300 (STFT -> magnitude
 * -> NMF -> float write-back with H/max(H)), without a host round trip in between.
 * audio: n host floats, element stride `stride`.
 * bases_seed: K x F floats or NULL (basesMode Seed/Fixed);  acts_seed: K x T floats or NULL
 * (channel-major like BufferAdaptor::samps(channel)).
 * bases_out: K x F floats or NULL;  acts_out: K x T floats or NULL (already scaled by
 * float(1/max H) in float arithmetic, :297-298);  resynth_out: K x n floats or NULL
 * (resynthMode 1, :302-334). */
int fluhip_bufnmf_channel_f32(fluhip_ctx* ctx, const float* audio, int64_t n, int64_t stride,
                              int64_t win, int64_t fft, int64_t hop, int64_t K, int64_t iters,
                              int update_w, int update_h, int64_t seed, const float* bases_seed,
                              const float* acts_seed, float* bases_out, float* acts_out,
                              float* resynth_out, fluhip_progress_fn progress, void* user);

/* ---- client::bufstft::BufferSTFTClient ----------------------------------------------------------- */
/* Replaces processFwd, clients/nrt/BufSTFTClient.hpp:81-184: padding_mode None/Default/Full = 0/1/2
 * (padding = 0, win/2, win-hop: clients/common/ParameterTypes.hpp:315-323), hops = 1 + (padded - win)/hop,
 * frame i = padded[i*hop, i*hop + win).  mag / phase (either may be NULL): bins x hops floats, one bin per
 * buffer channel like mags.allFrames().transpose() <<= tmpMags (:168-178). */
int fluhip_bufstft_forward_f32(fluhip_ctx* ctx, const float* audio, int64_t n, int64_t stride, int64_t win,
                               int64_t fft, int64_t hop, int padding_mode, float* mag, float* phase,
                               int64_t* hops_out);
/* Replaces processInverse, :186-276: std::polar(mag, phase) -> ISTFT::processFrame -> overlap-add /
 * window^2 normaliser -> drop `padding` leading samples.  out: (hops-1)*hop + win - padding floats
 * (call with out == NULL to query *n_out). */
int fluhip_bufstft_inverse_f32(fluhip_ctx* ctx, const float* mag, const float* phase, int64_t hops, int64_t win,
                               int64_t fft, int64_t hop, int padding_mode, float* out, int64_t* n_out);

/* ---- algorithm::NMFCross / GriffinLim, client::nmfcross::NMFCrossClient (BufNMFCross) ------------------------- */
/* Added within version 5: these three exports are additive, nothing of the version-5 ABI changed meaning.
 * NMFCross(iters) + addProgressCallback + process(X, H1, W0, r, p, c, seed)  (algorithms/public/NMFCross.hpp:46-78,
 * 156-186): X T x F (ldx), W0 K x F (ldw, read only), H1 T x K.  1 <= p <= K, r, c >= 1.  progress(1..iters), returning 0
 * cancels (FLUHIP_CANCELLED; the device is at most fluhip_ctx_set_progress_lag iterations ahead, 8 by default).
 * The reference's constraint factor is 1 - ((i + 1) / iters) in INTEGER arithmetic (:132, :150): 1 on every iteration but
 * the last and 0 on the last, so the temporal-sparsity and polyphony constraints leave H unchanged until iteration
 * iters - 1 and there zero every entry they do not keep (with iters == 1: on iteration 0).  Reproduced as such.
 * Polyphony ties (std::sort is not stable, :79-86) go to the lower source frame.  FP64 throughout; the quotients are
 * correctly rounded divisions. */
int fluhip_nmfcross_process_f64(fluhip_ctx* ctx, const double* X, int64_t T, int64_t F, int64_t ldx, const double* W0,
                                int64_t K, int64_t ldw, int64_t time_sparsity, int64_t polyphony, int64_t continuity,
                                int64_t iters, int64_t seed, double* H1, fluhip_progress_fn progress, void* user);
/* GriffinLim::process (algorithms/public/GriffinLim.hpp:26-52): spec T x F interleaved complex, in and out;
 * T == (n_samples + hop) / hop.  Hann window; the random phase is the reference's column-major T x F fill. */
int fluhip_griffinlim_f64(fluhip_ctx* ctx, double* spec, int64_t T, int64_t F, int64_t n_samples, int64_t iters,
                          int64_t win, int64_t fft, int64_t hop, int64_t seed);
/* NMFCrossClient::process (clients/nrt/NMFCrossClient.hpp:84-184), channel 0 of each buffer, the whole job on the device:
 * STFT of both, NMFCross with polyphony min(source frames, polyphony), synthesis, GriffinLim (50 iterations), ISTFT.
 * out: n_tgt floats (the reference resizes its output to n_tgt x 1 at the SOURCE's sample rate).  The reference's
 * messages in its order: "Empty source buffer", "Empty target buffer", "Time Sparsity is larger than target frames",
 * "Continuity is larger than target frames".  progress(1..iters) in the loop, then iters+1 / +2 / +3 after synthesis /
 * Griffin-Lim / ISTFT; returning 0 cancels (FLUHIP_CANCELLED, out unwritten). */
int fluhip_bufnmfcross_f32(fluhip_ctx* ctx, const float* source, int64_t n_src, int64_t src_stride, const float* target,
                           int64_t n_tgt, int64_t tgt_stride, int64_t win, int64_t fft, int64_t hop,
                           int64_t time_sparsity, int64_t polyphony, int64_t continuity, int64_t iters, int64_t seed,
                           float* out, fluhip_progress_fn progress, void* user);

/* Diagnostic: the form the NMFCross GEMMs (GEMM1 T x F over K, GEMM2 T x K over F, synthesis T x 2F over K) take for an
 * M x N output over a contraction of Kd on this context's device: out3 = {1: 128 x 128 workgroup tiles / 0: 64 x 64,
 * contraction splits, split depth}.  What the tests assert the forms they exercise by. */
int fluhip_debug_cross_plan(fluhip_ctx* ctx, int64_t M, int64_t N, int64_t Kd, int64_t* out3);
/* Diagnostic: one constraint stencil of the NMFCross H loop, the launch the clients share, on the caller's doubles.
 * H and out are T x K (frames x source frames, row-major).  which 0: promoteContinuity, size = continuity; 1:
 * enforceTemporalSparseness on the iteration where its factor is 0, size = time sparsity; 2: restrictPolyphony on that
 * iteration, size = polyphony <= K, energy[K] required (ignored otherwise).  Null H / out, T or K < 1, size < 1 (or above
 * 1048576) and polyphony > K are FLUHIP_ERROR with a message.  What tests/test_gpu_nmfcross.py holds bit for bit. */
int fluhip_debug_cross_stencil_f64(fluhip_ctx* ctx, const double* H, int64_t T, int64_t K, int which, int64_t size,
                                   const double* energy, double* out);

/* ---- algorithm::Novelty / NoveltyFeature / NoveltySegmentation, clients BufNoveltySlice / BufNoveltyFeature ---- */
/* Added within version 5 (additive).  FP64 throughout, every buffer of a call in the same launches.
 * kernel_size odd and >= 3 (at most 32767), 1 <= filter_size <= 1048576, threshold >= 0, min_slice >= 0: anything else
 * is FLUHIP_ERROR with a message and no output written.
 *
 * NoveltyFeature::processFrame over all frames (algorithms/public/NoveltyFeature.hpp:44-62 on util/Novelty.hpp:48-100):
 * feat `count` x T x D doubles (row stride ld >= D, buffer stride T ld) -> curve count x T.  filter_size 1 gives the raw
 * Novelty::processFrame output.  The gaussian of the checkerboard kernel has sigma = kernel_size / 3 in INTEGER
 * arithmetic, as the reference's (algorithms/public/WindowFuncs.hpp:66-73).  feat and curve may both be device
 * pointers: they are then used in place. */
int fluhip_novelty_curve_f64(fluhip_ctx* ctx, const double* feat, int64_t count, int64_t T, int64_t D, int64_t ld,
                             int64_t kernel_size, int64_t filter_size, double* curve);
/* NoveltySegmentation::processFrame over all frames (algorithms/public/NoveltySegmentation.hpp:44-63): det count x T
 * bytes (1 where the call for that frame returns a detection -- one frame behind the peak it reports), counts [count]
 * detections per buffer; curve (count x T, may be NULL) as above. */
int fluhip_novelty_slices_f64(fluhip_ctx* ctx, const double* feat, int64_t count, int64_t T, int64_t D, int64_t ld,
                              int64_t kernel_size, int64_t filter_size, double threshold, int64_t min_slice,
                              unsigned char* det, int64_t* counts, double* curve);
/* NRTNoveltySliceClient (clients/rt/NoveltySliceClient.hpp behind NRTSliceAdaptor, clients/common/
 * FluidNRTClientWrapper.hpp:665-725, SpikesToTimes.hpp) for `count` equal-length buffers: audio [count][channels][n]
 * floats, the channels summed in float; frame i holds the samples [i hop - win, i hop) of the sum followed by zeros
 * (FluidSource / BufferedProcess at the wrapper's host vector of 64), a detection of frame i stands at sample i hop;
 * detections inside the first latency = hop (1 + ((kernel_size + 1) >> 1) + (filter_size rounded up to even >> 1))
 * samples become ONE at 0, the others are reported as sample - latency + start_frame while below n.
 * algorithm: 0 Spectrum (STFT magnitudes, D = fft / 2 + 1), 1 MFCC (40 mel bands 20 Hz .. 20 kHz, 13 coefficients from
 * c0, in double).  2 Chroma, 3 Pitch, 4 Loudness are NOT built: FLUHIP_ERROR, the message names the algorithm, nothing
 * is written.  indices [count][capacity], counts [count] = the TRUE number of values of each buffer (values past
 * `capacity` are not written); a buffer without detection has count 1 and the single value -1.  Silence gives that for
 * Spectrum.  For MFCC it gives ONE slice at start_frame, as the reference's arithmetic does: the MFCC rows of silence
 * are constant and non-zero (20 log10(eps) in every band) against the zeros the ring of frames starts with, the curve
 * peaks at frame 1 (0.857 at kernel_size 3), inside the latency.
 * filter_size is at most 1048576 here. */
int fluhip_bufnoveltyslice_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n,
                               int64_t start_frame, int algorithm, int64_t kernel_size, double threshold,
                               int64_t filter_size, int64_t min_slice, int64_t win, int64_t fft, int64_t hop,
                               double sample_rate, int64_t* indices, int64_t capacity, int64_t* counts);
/* NRTNoveltyFeatureClient (clients/rt/NoveltyFeatureClient.hpp behind StreamingControl, FluidNRTClientWrapper.hpp:551-660)
 * for `count` equal-length mono buffers: one float per hop, the first latency / hop values dropped; padding_mode
 * 0 / 1 / 2 as the other *_padded_* calls.  out [count][*frames_out] (out == NULL: only *frames_out is set).
 * algorithm as above. */
int fluhip_bufnoveltyfeature_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int algorithm,
                                 int64_t kernel_size, int64_t filter_size, int64_t win, int64_t fft, int64_t hop,
                                 double sample_rate, int padding_mode, float* out, int64_t* frames_out);
/* Diagnostic: how the novelty curve of T frames of D dimensions is computed at a kernel size: out3 = {form, feature rows
 * a workgroup holds, curve values it writes}; form 0: band on chip, Gram blocks on the FP64 matrix pipe; 1: band on chip,
 * plain FMAs (D < 32); 2: tiled through a workspace in memory (kernel_size > 65). */
int fluhip_debug_novelty_plan(fluhip_ctx* ctx, int64_t T, int64_t D, int64_t kernel_size, int64_t* out3);

/* ---- algorithm::OnsetDetectionFunctions / OnsetSegmentation, clients BufOnsetSlice / BufOnsetFeature ---- */
/* Added within version 5 (additive).  FP64 throughout, every buffer of a call in the same launches.
 * function (the reference's "metric") 0 Energy, 1 High Frequency Content, 2 Spectral Flux, 3 Modified Kullback-Leibler,
 * 4 Itakura-Saito, 5 Cosine, 6 Phase Deviation, 7 Weighted Phase Deviation, 8 Complex Domain, 9 Rectified Complex Domain;
 * filter_size odd in [1, 101]; frame_delta in [0, 8192]; win >= 1, hop >= 1, fft a power of two in [max(4, win), 65536];
 * threshold >= 0, min_slice >= 0.  Anything else is FLUHIP_ERROR with a message that names the parameter; nothing is
 * clamped and no output is written.
 *
 * The algorithm-level calls take `count` signals of n doubles (stride ld >= n) that the caller has padded already:
 * frame i reads the samples [i hop, i hop + win + d), d = frame_delta for functions 2, 3, 4 and 0 otherwise (the other
 * functions ignore frame_delta, as the reference does); samples past n read as zero.  A frame is win samples times a
 * Hann window, zero-padded at the tail to fft.  With d != 0 the function compares the transform of the samples
 * [d, d + win) of the slice with that of its first win samples; otherwise the frame with the one or two frames before
 * it, zero spectra before frame 0.  The "phase" of functions 6 .. 9 is the real part of the complex arctangent of a bin,
 * as the reference's (util/OnsetDetectionFuncs.hpp:82-128), and wrapPhase is kept as written there.
 *
 * OnsetDetectionFunctions::processFrame over T frames (algorithms/public/OnsetDetectionFunctions.hpp:70-114): raw
 * count x T function values, filtered count x T = raw minus the median of the last filter_size values (zeros before the
 * start, the value of rank filter_size / 2); below filter_size 3 the reference subtracts a member it never sets and
 * filtered equals raw.  Either output may be NULL. */
int fluhip_onset_curve_f64(fluhip_ctx* ctx, const double* signal, int64_t count, int64_t n, int64_t ld, int64_t T, int64_t win,
                           int64_t fft, int64_t hop, int function, int64_t filter_size, int64_t frame_delta, double* raw,
                           double* filtered);
/* OnsetSegmentation::processFrame over T frames (algorithms/public/OnsetSegmentation.hpp:46-66): det count x T bytes, 1
 * where filtered > threshold with the previous filtered value (0 before frame 0) below it and the debounce counter at
 * zero; a detection sets the counter to min_slice, every other frame lowers it by one while positive.  counts [count]
 * detections per signal; filtered (count x T) may be NULL. */
int fluhip_onset_slices_f64(fluhip_ctx* ctx, const double* signal, int64_t count, int64_t n, int64_t ld, int64_t T, int64_t win,
                            int64_t fft, int64_t hop, int function, int64_t filter_size, int64_t frame_delta, double threshold,
                            int64_t min_slice, unsigned char* det, int64_t* counts, double* filtered);
/* NRTOnsetSliceClient (clients/rt/OnsetSliceClient.hpp behind NRTSliceAdaptor, clients/common/
 * FluidNRTClientWrapper.hpp:665-725, SpikesToTimes.hpp) for `count` equal-length buffers: audio [count][channels][n]
 * floats, the channels summed in float.  The derivation: the wrapper appends the client's latency -- one hop
 * (OnsetSliceClient::latency) -- of zeros and rounds the length up to whole host vectors of 64; BufferedProcess fires a
 * frame at every multiple i hop below that length, and FluidSource::pull hands it the W = win + d samples that END
 * there (d = frame_delta for functions 2, 3, 4: OnsetSliceClient::process :89-91), so frame i holds [i hop - W, i hop)
 * of the sum, zeros outside; the client writes the detection at sample i hop (mFrameOffset).  Detections inside the
 * first `hop` samples -- frames 0 and 1 -- become ONE at 0, the others are reported as i hop - hop + start_frame while
 * below n.  For d = 0 this is the framing of the reference's SlicerTestHarness (signal one window in, positions
 * i hop - hop), whose expected positions the algorithm-level call reproduces.
 * indices [count][capacity], counts [count] = the TRUE number of values of each buffer (values past `capacity` are
 * not written); a buffer without detection has count 1 and the single value -1. */
int fluhip_bufonsetslice_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n,
                             int64_t start_frame, int function, double threshold, int64_t min_slice, int64_t filter_size,
                             int64_t frame_delta, int64_t win, int64_t fft, int64_t hop, int64_t* indices, int64_t capacity,
                             int64_t* counts);
/* NRTOnsetFeatureClient (clients/rt/OnsetFeatureClient.hpp behind StreamingControl, FluidNRTClientWrapper.hpp:551-660)
 * for `count` equal-length mono buffers: one float per hop (the filtered value), the first latency / hop = 1 value
 * dropped; padding_mode 0 / 1 / 2 as fluhip_bufnoveltyfeature_f32, computed from win (OnsetFeatureClient::
 * analysisSettings; the frame delta is not part of it).  Frame j holds the samples [j hop - W - pad, j hop - pad).
 * out [count][*frames_out] (out == NULL: only *frames_out is set). */
int fluhip_bufonsetfeature_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int function,
                               int64_t filter_size, int64_t frame_delta, int64_t win, int64_t fft, int64_t hop,
                               int padding_mode, float* out, int64_t* frames_out);
/* Diagnostic: how the onset curve is computed at (fft, win, function, frame_delta) -- nothing else enters: out4 = {form,
 * frames of history recomputed in front of a run (0, 1 or 2), transforms per frame (2 with a frame delta), frames a
 * workgroup writes}.  form 0: one fused launch -- a workgroup transforms a run of 32 consecutive frames of one buffer on
 * chip, keeps their spectra in the LDS and writes one double per frame; built where the project's on-chip FFT core is:
 * fft 1024, 2048 and 4096 with an even window.  form 1: two passes, the STFT launch writes a round's complex spectra to a
 * workspace and the reduction reads them (every other shape; run 0). */
int fluhip_debug_onset_plan(fluhip_ctx* ctx, int64_t fft, int64_t win, int function, int64_t frame_delta, int64_t* out4);

/* ---- algorithm::HPSS, client BufHPSS (harmonic / percussive separation by median filtering) ---- */
/* Added within version 5 (additive).  FP64 throughout, every buffer of a call in the same launches.
 * harm_filter_size and perc_filter_size odd in [3, 1001], perc_filter_size <= bins; mode 0 Classic, 1 Coupled, 2 Advanced;
 * harm_thresh / perc_thresh: four doubles (x1, y1, x2, y2), frequencies x as fractions of the bins in [0, 1] with x1 <= x2,
 * amplitudes y in dB (the reference's default is (0, 1, 1, 1); its FrequencyAmpPairConstraint, which clips and swaps, is the
 * client's).  Anything else is FLUHIP_ERROR with a message that names the parameter; nothing is clamped and no output is
 * written.
 *
 * HPSS::processFrame (algorithms/public/HPSS.hpp:66-152) is a streaming routine with history; over a whole plane whose
 * row t is the t-th frame it computes, with h2 = (harm_filter_size - 1) / 2 and a median being the value of rank size / 2:
 *   vmed[t][f]  the median of the bins f .. f + perc_filter_size - 1 of row t, zeros past the last bin (forward-looking);
 *   hmed[t][f]  the median of bin f over the rows t - h2 - 1 .. t + h2 - 1, zeros outside 0 .. T - 1 (centred ONE ROW BEFORE t);
 *   mode 0      mult = 1 / max(hmed + vmed, eps): masks hmed mult, vmed mult, 0
 *   mode 1      harmonic = (hmed / vmed > threshold_h[f]) as 0 / 1, percussive = 1 - harmonic, residual 0
 *   mode 2      harmonic as in mode 1, percussive = (vmed / hmed > threshold_p[f]), residual = (1 - harmonic)(1 - percussive),
 *               all three times max(1 / (their sum), eps)
 * every mask through min(1, .); 0 / 0 compares false, x / 0 true.  threshold[f] is HPSS::makeThreshold (:157-174):
 * 10^(y1 / 20) below bin floor(x1 bins), 10^(y2 / 20) from bin floor(x2 bins) on, 10^(LinSpaced(y1, y2) / 20) between.
 * The medians are selections: they are the bits of a sort of the same magnitudes.
 *
 * mag count x T x ld doubles (ld >= F); hmed, vmed and the three entries of masks (harmonic, percussive, residual) are
 * count x T x F each; any of them, and masks itself, may be NULL. */
int fluhip_hpss_planes_f64(fluhip_ctx* ctx, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld,
                           int64_t harm_filter_size, int64_t perc_filter_size, int mode, const double* harm_thresh,
                           const double* perc_thresh, double* hmed, double* vmed, double* const* masks);
/* NRTHPSSClient (clients/rt/HPSSClient.hpp behind Streaming, clients/common/FluidNRTClientWrapper.hpp:466-547) for
 * `count` equal-length mono buffers: audio count x n floats, out count x 3 x n floats (harmonic, percussive, residual; the
 * residual is always written and is zeros in modes 0 and 1).  The wrapper drops the client's latency
 * (harm_filter_size - 1) hop + win, which puts every frame back where it came from: frame m = 1, 2, ... covers the samples
 * [m hop - win, m hop) (Hann window, zero-padded to fft), the planes above are taken over the frames that touch the buffer,
 * each masked spectrum is transformed back, windowed, overlap-added and divided by the overlap-added window^2.
 * hop <= win; fft a power of two in [max(4, win), 65536]. */
int fluhip_bufhpss_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft, int64_t hop,
                       int64_t harm_filter_size, int64_t perc_filter_size, int mode, const double* harm_thresh,
                       const double* perc_thresh, float* out);
/* Diagnostic: how the masks are computed at (harm_filter_size, perc_filter_size) -- nothing else enters: out4 = {form of
 * the harmonic median, form of the percussive median, bytes of LDS a workgroup takes, bins a workgroup owns (256)}.  form 0:
 * the filter's window is copied to the LDS once and ranked from there (sizes up to 63); form 1: ranked straight from the
 * plane in memory.  ctx may be NULL (no device is used). */
int fluhip_debug_hpss_plan(fluhip_ctx* ctx, int64_t harm_filter_size, int64_t perc_filter_size, int64_t* out4);

/* ---- BufPitch (clients/rt/PitchClient.hpp: YinFFT, harmonic product spectrum, cepstrum) -------- */
/* algorithm::CepstrumF0 (0), HPS with nHarmonics = 4 (1) or YINFFT (2) ::processFrame on every frame of `count` magnitude
 * planes: mag count x T x ld doubles (ld >= F, F = fft / 2 + 1 of a power-of-two fft), out count x T x 2 doubles
 * (pitch in Hz, confidence).  The reference's behaviour is kept: HPS multiplies mag[j] mag[2 j] mag[3 j] (its loop stops
 * before nHarmonics), YinFFT clamps its lag range to [min(lrint(sr / max_freq), F - 1), min(lrint(sr / min_freq),
 * F - minBin - 1)) and takes a frequency of 0 as 1, peaks are the local maxima above the segment's minimum, ordered by
 * their parabolically interpolated height (equal heights: the lowest index).  Where the reference reads past its arrays
 * the range is clamped: HPS searches [minBin, min(maxBin, F)), and a quotient sr / freq at or beyond F counts as F before
 * it is rounded.  Cepstrum needs fft <= 8192 (its DCT table is F x F).  YinFFT takes a squared magnitude at or below
 * DBL_MIN as zero, here as in fluhip_bufpitch_f32, whose transform returns sqrt(DBL_MIN) for an exactly zero bin (the
 * reference does not flush; such magnitudes lie 150 orders of magnitude below any sample a float carries). */
int fluhip_pitch_frames_f64(fluhip_ctx* ctx, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld, int algorithm,
                            double min_freq, double max_freq, double sample_rate, double* out);
/* Diagnostic: the curve the algorithm searches, count x T x F doubles: the normalised yin (NaN in an all-zero frame, as
 * in the reference), the harmonic product, or the whole cepstrum. */
int fluhip_debug_pitch_curve_f64(fluhip_ctx* ctx, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld,
                                 int algorithm, double min_freq, double max_freq, double sample_rate, double* curve);
/* NRTPitchClient (PitchClient behind StreamingControl, clients/common/FluidNRTClientWrapper.hpp:551-660) for `count`
 * equal-length mono buffers: audio count x n floats; padding_mode as in fluhip_bufmfcc_padded_f32; the client's latency
 * is win.  unit 0: Hz, 1: MIDI (69 + 12 log2(x / 440), -999 for 0).  select: bit 0 pitch, bit 1 confidence; the selected
 * values are the output channels in that order: out count x selected x frames floats; select 0 is an error.  With out
 * NULL only *frames_out is written (size query).  sample_rate is the source buffer's. */
int fluhip_bufpitch_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft, int64_t hop,
                        int padding_mode, int algorithm, double min_freq, double max_freq, int unit, int select,
                        double sample_rate, float* out, int64_t* frames_out);
/* Diagnostic: how (fft, win, algorithm) is computed: out4 = {form, frames a workgroup of the on-chip form writes,
 * transforms per frame, rows of the cepstrum's DCT table that are multiplied at the default bounds and 44.1 kHz (0 for the
 * other algorithms)}.  form 0: transform and pitch in one launch, a run of 32 frames per workgroup, the magnitudes stay in
 * the LDS -- fft 1024, 2048 and 4096 with an even window.  form 1: the STFT launch leaves a round's magnitudes in a
 * workspace, the pitch kernels read them (run 0). */
int fluhip_debug_pitch_plan(fluhip_ctx* ctx, int64_t fft, int64_t win, int algorithm, int64_t* out4);

/* ---- BufSpectralShape, BufChroma (clients/rt/SpectralShapeClient.hpp, clients/rt/ChromaClient.hpp) -------- */
/* algorithm::SpectralShape::processFrame on every frame of `count` magnitude planes: mag count x T x ld doubles (ld >= F,
 * F = fft / 2 + 1 of a power-of-two fft from 4 to 65536), out count x T x 7 doubles: centroid, spread, skewness, kurtosis,
 * rolloff, flatness, crest.  The reference's behaviour is kept:
 *   - mag = max(mag, epsilon) comes before anything else;
 *   - binHz = sr / (2 (F - 1)), minBin = ceil(min_freq / binHz), maxBin = min(floor(max_freq / binHz), F - 1), max_freq -1
 *     meaning sr / 2 and anything above it capped there; maxBin <= minBin gives seven zeros;
 *   - unit 1 (MIDI) with minBin 0: minBin becomes 1 and bin 1 takes bin 0's magnitude too;
 *   - the segment is the maxBin - minBin bins minBin .. maxBin - 1 (bin maxBin is never read), yet its frequency axis is
 *     LinSpaced(size, minBin binHz, maxBin binHz): the step is (maxBin - minBin) binHz / (size - 1), not binHz, and a
 *     segment of one bin sits at maxBin binHz; the MIDI axis is 69 + 12 log(f / 440) log2E;
 *   - the moments are sums about the centroid; the spread is returned as its square root, skewness and kurtosis divide by
 *     powers of the unrooted spread;
 *   - the rolloff is the first bin at which the running sum reaches rolloff_percent of the total, interpolated linearly
 *     inside that bin (the first bin: its own frequency); if the sum never gets there the result is maxBin - 1, a bin
 *     index.  rolloff_percent 100 depends on the order of summation in the reference itself and is not pinned: either the
 *     last frequency step or maxBin - 1;
 *   - flatness is 20 log10(max(exp(mean(log amp)) / mean(amp), epsilon)), crest 20 log10(max(max(amp) / mean(amp),
 *     epsilon)); power 1 squares the clamped magnitudes.
 * Defined here where the reference leaves its arrays: a quotient freq / binHz at or beyond F counts as F, and the segment
 * the MIDI axis leaves empty (minBin 0 -> 1, maxBin 1) gives seven zeros.  Errors (nothing is clamped, nothing is written):
 * min_freq < 0, max_freq < -1, rolloff_percent outside [0, 100], unit or power outside {0, 1}, a sample_rate that is not
 * positive and finite, an fft that is no power of two in [4, 65536].  mag and out are host pointers. */
int fluhip_spectralshape_frames_f64(fluhip_ctx* ctx, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld,
                                    double min_freq, double max_freq, double rolloff_percent, int unit, int power,
                                    double sample_rate, double* out);
/* NRTSpectralShapeClient (SpectralShapeClient behind StreamingControl, clients/common/FluidNRTClientWrapper.hpp:551-660) for
 * `count` equal-length mono buffers: audio count x n floats; padding_mode as in fluhip_bufmfcc_padded_f32; the client's
 * latency is win, and the frames inside it are dropped without being transformed.  select: bits 0 .. 6 = centroid, spread,
 * skew, kurtosis, rolloff, flatness, crest, in [1, 127]; the selected descriptors are the output channels in that order:
 * out count x selected x frames floats (host).  With out NULL only *frames_out is written (size query).  sample_rate is
 * the source buffer's.  The block STFT hands an exactly zero bin over as sqrt(DBL_MIN); the clamp to epsilon comes first,
 * so digital silence is the all-epsilon frame of the reference. */
int fluhip_bufspectralshape_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft,
                                int64_t hop, int padding_mode, int select, double min_freq, double max_freq,
                                double rolloff_percent, int unit, int power, double sample_rate, float* out, int64_t* frames_out);
/* Diagnostic: the table of algorithm::ChromaFilterBank::init, out num_chroma x F doubles.  As the reference builds it:
 * fftSize = 2 (F - 1); freqs = LinSpaced(fftSize, 0, sr), i.e. fftSize points with the step sr / (fftSize - 1) and not
 * sr / fftSize; then num_chroma log(freqs / (ref / 16)) log2E, freqs[0] = freqs[1] - 1.5 num_chroma; widths are the
 * successive differences floored at 1; halfChroma = num_chroma / 2 in integers; the remainder is C's fmod(d + 10 num_chroma
 * + halfChroma, num_chroma) - halfChroma, which goes negative for a large ref at a large fft; the weights are
 * exp(-0.5 (2 r / width)^2), only the first F columns are kept and each is divided by its L2 norm over the rows. */
int fluhip_debug_chroma_filters_f64(fluhip_ctx* ctx, int64_t num_chroma, int64_t F, double ref, double sample_rate, double* out);
/* algorithm::ChromaFilterBank::processFrame on every frame of `count` magnitude planes (mag as above, never modified:
 * the reference zeroes its caller's frame in place), out count x T x num_chroma doubles.  The range branch runs only if
 * min_freq != 0 or max_freq != -1; inside it minBin = 0 for min_freq 0, else ceil(min_freq / binHz), maxBin =
 * min(floor(min(max_freq, sr / 2) / binHz), F - 1), the bins 0 .. minBin INCLUSIVE and maxBin .. F - 1 are zeroed (both runs
 * clamped to the frame).  Then the squares, the product with the filter table, times 2 / (fftSize num_chroma); normalize 1
 * divides by max(sum, epsilon), 2 by max(max, epsilon).  A squared magnitude at or below DBL_MIN counts as zero, here as
 * in fluhip_bufchroma_f32, whose block transform returns sqrt(DBL_MIN) for an exactly zero bin: silence is exactly 0.
 * Errors: num_chroma outside [2, 128], ref outside (0, 22000], normalize outside {0, 1, 2}, min_freq < 0, a max_freq that is
 * neither -1 nor >= 0 (the reference indexes at -1 in between), sample_rate and fft as above. */
int fluhip_chroma_frames_f64(fluhip_ctx* ctx, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld,
                             int64_t num_chroma, double ref, int normalize, double min_freq, double max_freq, double sample_rate,
                             double* out);
/* NRTChromaClient (ChromaClient behind StreamingControl) for `count` equal-length mono buffers, framed as
 * fluhip_bufspectralshape_f32: out count x num_chroma x frames floats (host); out NULL is the size query. */
int fluhip_bufchroma_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft, int64_t hop,
                         int padding_mode, int64_t num_chroma, double ref, int normalize, double min_freq, double max_freq,
                         double sample_rate, float* out, int64_t* frames_out);
/* Diagnostic: how (fft, win, kind) is computed, kind 0 SpectralShape, 1 Chroma: out4 = {form, frames a workgroup of the
 * on-chip form writes, transforms per frame (1), whether a GEMM with the filter table follows}.  form 0: transform and
 * descriptors (or Chroma's squared magnitudes) in one launch, a run of 32 frames per workgroup, the magnitudes stay in the
 * LDS -- fft 1024, 2048 and 4096 with an even window.  form 1: the STFT launch leaves a round's magnitudes in a workspace,
 * the kernels read them (run 0). */
int fluhip_debug_spectral_plan(fluhip_ctx* ctx, int64_t fft, int64_t win, int kind, int64_t* out4);

/* ---- BufLoudness (clients/rt/LoudnessClient.hpp) ---------------------------------------------------------- */
/* algorithm::Loudness::processFrame (algorithms/public/Loudness.hpp:43-61) on the frames of `count` signals: x count x n
 * doubles (host), frame j = x[j hop .. j hop + win), T = 1 + (n - win) / hop frames per signal, out count x T x 2 doubles
 * (host): loudness = -0.691 + 10 log10(mean(filtered^2) + epsilon) and peak = 20 log10(peak + epsilon), epsilon DBL_EPSILON.
 * One Loudness object per signal, initialised once: the K-weighting filter (util/KWeightingFilter.hpp, the shelving and the
 * high-pass biquad as one 5-tap direct-form-I recursion, coefficients in double from the sample rate) is never reset between
 * frames, and the true-peak interpolator (util/TruePeak.hpp: 49 taps, Hann-windowed sinc, factor 4 below 88200 Hz, 2 from
 * there on, taps with |c| <= 1e-6 dropped) keeps its ring buffer of ceil(49 / factor) samples: both states are carried from
 * frame 0 through the overlapping frames, nothing is dropped.  The -0.691 stays when k_weighting is 0; the peak is taken from
 * the unfiltered frame; at 176400 Hz and above, and with true_peak 0, it is max |x|.  No state passes between signals: a
 * batch gives the bits of single calls.  hop > win is legal.
 * Errors: win outside [1, 32768], hop < 1, k_weighting / true_peak outside {0, 1}, a sample rate that is not positive and
 * finite, count < 1, n < win ("not enough frames"); nothing is written. */
int fluhip_loudness_frames_f64(fluhip_ctx* ctx, const double* x, int64_t count, int64_t n, int64_t win, int64_t hop, int k_weighting,
                               int true_peak, double sample_rate, double* out);
/* NRTLoudnessClient (LoudnessClient behind StreamingControl, clients/common/FluidNRTClientWrapper.hpp:551-660) for `count`
 * equal-length mono buffers of n float samples: padding_mode 0 None, 1 Default (win / 2), 2 Full (win - hop); the latency is
 * win; analysis frame j holds the win samples from j hop - win - padding of the input on (zeros outside it); every frame,
 * the latency frames included, runs through the filter and the interpolator, then the first win / hop results are dropped.
 * select bit 0 loudness, bit 1 peak; out count x selected x frames floats (host), *frames_out the kept frames; out NULL is the
 * size query.  Errors: as above, select outside [1, 3], padding_mode outside {0, 1, 2}, padding_mode 2 with hop > win (the
 * reference copies its input to a negative offset), no frame left. */
int fluhip_bufloudness_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t hop, int padding_mode,
                           int select, int k_weighting, int true_peak, double sample_rate, float* out, int64_t* frames_out);
/* Diagnostic: how (win, hop, sample rate) is computed: out4 = {form, frames a workgroup owns, interpolation factor (4 / 2 /
 * 1 = no interpolator), history samples of the frame stream the interpolator reads in front of a frame (ring - 1)}.  form 0:
 * lane = frame -- zero-state end states, a scan of 8-value states per buffer in double-double, every frame run again from its
 * entering state.  ctx may be NULL (an error then leaves no message). */
int fluhip_debug_loudness_plan(fluhip_ctx* ctx, int64_t win, int64_t hop, double sample_rate, int64_t* out4);

/* ---- BufAmpSlice / BufAmpFeature (clients/rt/AmpSliceClient.hpp, AmpFeatureClient.hpp) ---------------------- */
/* Added within version 5 (additive).  FP64 throughout, every signal of a call in the same launches; there are no frames:
 * every sample depends on the one before.
 * algorithm::Envelope::processSample (algorithms/public/Envelope.hpp:36-61) over `count` signals: x count x n doubles
 * (host), rows ld apart; out count x n doubles (host).  One Envelope object per signal, initialised once.  Per sample: a
 * sample that is not finite is replaced by the last finite one (0 before the first); two identical second-order Butterworth
 * high-pass sections in cascade (util/ButterworthHPFilter.hpp: direct form I, zero initial state, coefficients in double from
 * hipass = the cutoff as a fraction of the sample rate, the recursion evaluated left to right; hipass 0 bypasses them);
 * 20 log10 |.|, then max(., floor_db) (a zero gives -inf, which becomes the floor); two SlideUDFilters (util/
 * SlideUDFilter.hpp) that both start at floor_db, take 1 / ramp_up when the input is strictly above their state and
 * 1 / ramp_down otherwise, and move by y0 + (b * (x - y0)) in three roundings; the value is fast - slow.
 * The front end up to the clipped level is computed in chunks of 1024 samples whose entering filter states come from a scan
 * (carried in double-double), every chunk then run in plain double in the reference's order; the followers run serially, a
 * lane pair per signal.  Nothing depends on count or on n: a batch gives the bits of single calls.
 * Errors: a ramp below 1, floor_db outside [-144, 144], hipass outside [0, 0.5], count < 1, n < 1, ld < n; the message names
 * the parameter, nothing is clamped and nothing is written. */
int fluhip_amp_envelope_f64(fluhip_ctx* ctx, const double* x, int64_t count, int64_t n, int64_t ld, int64_t fast_up,
                            int64_t fast_down, int64_t slow_up, int64_t slow_down, double floor_db, double hipass, double* out);
/* algorithm::EnvelopeSegmentation::processSample (algorithms/public/EnvelopeSegmentation.hpp:36-60) over the same envelope:
 * det count x n bytes (host, may be NULL), 1 where a slice starts; counts (count) how many; envelope count x n doubles (may
 * be NULL).  The previous value starts at 0; a detection needs !state && value > on && previous < on && debounce == 0, all
 * strict; it sets the debounce counter to min_slice (0 is legal), and the counter is lowered only on samples that do not
 * detect; state falls when value < off, tested after the detection on the same sample.
 * Errors: as above, on / off outside [-144, 144], min_slice < 0. */
int fluhip_amp_slices_f64(fluhip_ctx* ctx, const double* x, int64_t count, int64_t n, int64_t ld, int64_t fast_up, int64_t fast_down,
                          int64_t slow_up, int64_t slow_down, double on, double off, double floor_db, int64_t min_slice,
                          double hipass, unsigned char* det, int64_t* counts, double* envelope);
/* NRTAmpSliceClient (AmpSliceClient behind NRTSliceAdaptor, clients/common/FluidNRTClientWrapper.hpp:665-725) for `count`
 * buffers of `channels` x n float samples: the channels are summed in float, in channel order, starting from 0; hipass =
 * min(high_pass_freq / sample_rate, 0.5); the client's latency is 0, so no detection is moved or merged at the front, and the
 * zeros that fill the last host vector lie past n.  indices / capacity / counts / start_frame as fluhip_bufonsetslice_f32: at
 * most `capacity` values per buffer (start_frame added) at indices + b * capacity, counts[b] the true number; a buffer without
 * detection yields the single value -1.
 * Errors: as above, a negative or non-finite high_pass_freq, a sample rate that is not positive and finite, channels < 1. */
int fluhip_bufampslice_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n, int64_t start_frame,
                           int64_t fast_up, int64_t fast_down, int64_t slow_up, int64_t slow_down, double on, double off,
                           double floor_db, int64_t min_slice, double high_pass_freq, double sample_rate, int64_t* indices,
                           int64_t capacity, int64_t* counts);
/* NRTAmpFeatureClient (AmpFeatureClient behind NRTStreamAdaptor, FluidNRTClientWrapper.hpp:466-548): every channel on its own
 * through a reset client, latency 0; out count x channels x n floats (host), each value cast to float. */
int fluhip_bufampfeature_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n, int64_t fast_up,
                             int64_t fast_down, int64_t slow_up, int64_t slow_down, double floor_db, double high_pass_freq,
                             double sample_rate, float* out);
/* Diagnostic: how the envelope is computed at hipass -- nothing else enters: out4 = {form, samples of a front-end chunk,
 * signals per wavefront of the serial follower kernel, 1 if the high-pass scan launches run (hipass > 0)}.  form 0: lane =
 * chunk in the front end, a lane pair per signal behind it.  ctx may be NULL (an error then leaves no message). */
int fluhip_debug_amp_plan(fluhip_ctx* ctx, double hipass, int64_t* out4);

/* ---- BufAmpGate (clients/rt/AmpGateClient.hpp) --------------------------------------------------------------- */
/* The slicer that answers with onset / offset pairs: the sounding regions of a signal.
 * algorithm::EnvelopeGate::processSample (algorithms/public/EnvelopeGate.hpp:64-175) over `count` signals: x count x n doubles
 * (host), rows ld apart.  One EnvelopeGate object per signal, initialised once.  Per sample: the front end of
 * fluhip_amp_envelope_f64 (hold of the last finite sample, two Butterworth sections at hipass, 20 log10 |.|) clipped at
 * min(on, off) - 1 -- not at -144 --, then ONE follower (1 / ramp_up, 1 / ramp_down) that starts there, as does every value of
 * the history in front of the first sample.  Behind it a Schmitt trigger (>= on, <= off: not strict) with two counters, and the
 * output state: it goes on when the trigger has been on for min_above samples, and the onset moves to the FIRST minimum of the
 * look_back smoothed values in front of those; it goes off when the trigger has been off for max(min_below, look_ahead) samples,
 * and the offset moves to the first minimum of the look_ahead values from there on.  A lookup length below 2 searches nothing
 * (it answers start + length).  Output already decided is repainted from the moved position, as far back as the latency L =
 * max(min_above + look_back, max(min_below, look_ahead)) reaches.  min_slice / min_silence hold the output for that many samples
 * (counted from the trigger's own count); while they do, the trigger and its counters stand still, and the sample on which the
 * hold ends is evaluated.
 * out (count x n bytes, host): what processSample returns for each input sample, the decision of the sample L - 1 steps
 * earlier (0 in front of the first).  smoothed (count x n doubles, host; may be NULL): the follower's value of every sample.
 * A transition scans its lookup window: a signal that toggles every other sample costs n L / 2 reads.
 * Errors: a ramp or one of min_slice, min_silence, min_above, min_below below 1; look_back or look_ahead below 0; on / off
 * outside [-144, 144] or NaN; hipass outside [0, 0.5]; max_size < 1; L > max_size; count < 1, n < 1, ld < n.  The message names
 * the parameter, nothing is clamped and nothing is written. */
int fluhip_amp_gate_f64(fluhip_ctx* ctx, const double* x, int64_t count, int64_t n, int64_t ld, int64_t ramp_up, int64_t ramp_down,
                        double on, double off, int64_t min_slice, int64_t min_silence, int64_t min_above, int64_t min_below,
                        int64_t look_back, int64_t look_ahead, double hipass, int64_t max_size, unsigned char* out,
                        double* smoothed);
/* NRTAmpGateClient (AmpGateClient behind NRTAmpGate, clients/rt/AmpGateClient.hpp:135-188, SpikesToTimes.hpp) for `count`
 * buffers of `channels` x n float samples: the channels are summed in float, in channel order, starting from 0, into n + L
 * samples with a zero tail; hipass = min(high_pass_freq / sample_rate, 0.5); with o[i] the decision of sample i + 1, an onset
 * stands at 0 if o[0] is on, onsets and offsets at the rises and falls of o for i in 1 .. n - 2, an offset at n - 1 if o[n - 1]
 * is on.  indices (count x 2 x capacity int64, host): the onsets of buffer b at indices + (2 b) capacity, its offsets at
 * indices + (2 b + 1) capacity, at most `capacity` each, start_frame added; counts[b] the true number of pairs; a buffer that
 * never switches yields the single pair (-1, -1), as fluhip_bufampslice_f32 answers silence.  With capacity 0 indices may be
 * NULL (the counts alone).
 * Where the gate changes on the last sample (o[n - 2] != o[n - 1]) the two rows differ in number; the reference asserts there.
 * Here counts[b] is -1 and the rows of that buffer are untouched, the other buffers are unaffected, the call returns FLUHIP_OK
 * and fluhip_last_error names the (first such) buffer.
 * Errors: as above, a negative or non-finite high_pass_freq, a sample rate that is not positive and finite, channels < 1. */
int fluhip_bufampgate_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n, int64_t start_frame,
                          int64_t ramp_up, int64_t ramp_down, double on, double off, int64_t min_slice, int64_t min_silence,
                          int64_t min_above, int64_t min_below, int64_t look_back, int64_t look_ahead, double high_pass_freq,
                          double sample_rate, int64_t max_size, int64_t* indices, int64_t capacity, int64_t* counts);
/* Diagnostic: how the gate is computed behind the front end of fluhip_debug_amp_plan: out4 = {form, signals per wavefront of
 * the two serial kernels, samples of a row staged through the LDS at a time, where a lookup reads its window: 0 global memory,
 * 1 the LDS}.  form 0: three launches -- follower, state machine over the finished plane, painter.  ctx may be NULL. */
int fluhip_debug_ampgate_plan(fluhip_ctx* ctx, int64_t* out4);

/* ---- feature pipeline: BufMelBands / BufMFCC (BASELINE config 5) ------------------------------ */
/* Replaces, for `count` equal-length mono buffers at once, the offline-wrapped real-time clients
 *   NRTThreadedMelBandsClient  clients/rt/MelBandsClient.hpp:77-119  (MelBands::processFrame, alg/MelBands.hpp:79-97)
 *   NRTThreadedMFCCClient      clients/rt/MFCCClient.hpp:86-131      (+ DCT::processFrame, alg/DCT.hpp:65-75)
 * as driven by StreamingControl with the default padding (clients/common/FluidNRTClientWrapper.hpp:551-660):
 * T = 1 + (n + 2 (win/2))/hop - win/hop frames, frame k starting at sample (win/hop)*hop - win - win/2 + k*hop
 * (for hop | win: [k*hop - win/2, k*hop + win/2), T = n/hop + 1).
 * audio: count x n floats.  out: count x nFeatures x T floats, feature-major per buffer like
 * BufferAdaptor::samps(feature).  Either may be a host or a device pointer (a corpus that already sits in HBM
 * skips the PCIe copies, which otherwise dominate: config 5 moves 2.9 GB in).  window: Hann (the clients pass no
 * window type). */
int fluhip_bufmelbands_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win,
                           int64_t fft, int64_t hop, int64_t n_bands, double min_freq, double max_freq,
                           double sample_rate, int normalize, int scale_db, float* out, int64_t* frames_out);
int fluhip_bufmfcc_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft,
                       int64_t hop, int64_t n_bands, int64_t n_coefs, int64_t start_coeff, double min_freq,
                       double max_freq, double sample_rate, float* out, int64_t* frames_out);
/* The same with the wrapper's "padding" parameter (None / Default / Full = 0 / 1 / 2; the two calls above are mode 1):
 * userPadding = FFTParams::padding = 0 / win/2 / win - hop (clients/common/ParameterTypes.hpp:315-323,
 * FluidNRTClientWrapper.hpp:357-364), paddedLength = n + win + 2 userPadding, rounded up to whole hops in Full mode
 * (:572-574), T = 1 + (paddedLength - win)/hop - win/hop, kept frame k starting at sample
 * (win/hop) hop - win - userPadding + k hop. */
int fluhip_bufmelbands_padded_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win,
                                  int64_t fft, int64_t hop, int64_t n_bands, double min_freq, double max_freq,
                                  double sample_rate, int normalize, int scale_db, int padding_mode, float* out,
                                  int64_t* frames_out);
int fluhip_bufmfcc_padded_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft,
                              int64_t hop, int64_t n_bands, int64_t n_coefs, int64_t start_coeff, double min_freq,
                              double max_freq, double sample_rate, int padding_mode, float* out, int64_t* frames_out);
/* Diagnostic: the form BufMelBands (mfcc 0) / BufMFCC (mfcc 1) take at a shape -- a function of these parameters only; ctx
 * receives the message of a refusal and may be NULL.  out5 = {form, wavefronts per workgroup, frames per wavefront, bytes
 * of dynamic LDS, rows staged}.  form 0: one fused launch, STFT -> mel bands -> DCT with the magnitudes on chip (fft 1024
 * or 2048, an even window, at most 64 bands, a filter bank whose every bin lies on at most one rising and one falling
 * edge, and DCT rows that fit the kernel's LDS: at 64 bands 26 rows at fft 1024, 40 at fft 2048); the other four are 0.
 * form 1: the STFT launch, then the mel kernel over the magnitudes in memory in the layout the other four describe: 4, 2
 * or 1 wavefronts of 4 frames while that fits 160 KB of LDS, then 2 or 1 frames per wavefront, then (rows staged 0) the
 * magnitude rows read from memory instead of the LDS.  A band count whose energies alone do not fit (more than 20480
 * bands) is refused, here as in the calls themselves.  What the tests assert the forms they exercise by. */
int fluhip_debug_features_plan(fluhip_ctx* ctx, int mfcc, int64_t win, int64_t fft, int64_t n_bands, int64_t n_coefs,
                               int64_t start_coeff, double min_freq, double max_freq, double sample_rate, int64_t* out5);

/* ---- the users of NMF::processFrame: NMFMatch and NMFFilter ------------------------------------------------------------
 * clients/rt/NMFMatchClient.hpp:76-118 and clients/rt/NMFFilterClient.hpp:69-118 are real-time clients: a host vector in, a
 * host vector out, one NMF::processFrame per hop against the dictionary in the `bases` buffer.  These two calls are those
 * clients over a whole buffer, as the reference's offline wrapper templates drive a real-time client
 * (clients/common/FluidNRTClientWrapper.hpp: StreamingControl :551-660, Streaming :466-547) -- every frame of every channel
 * in one batch.  audio: count x n host floats (channels of one job; the client is reset per channel, :602 / :515).
 * bases: K x F host floats, F = fft/2 + 1 (the filter buffer's channels, K = min(channels, maxComponents)).
 *
 * fluhip_nmfmatch_f32 -- the control output of NMFMatch per hop: out[channel][component][T], T as for the feature clients
 * (fluhip_bufmfcc_padded_f32; *frames_out, also with out == NULL as a size query).  The client writes its output BEFORE
 * it processes the call's frame (:104 against :108-117), so column k holds the activations of the frame at audio sample
 * (k + win/hop - 1) hop - win - userPadding: one hop behind the frame BufMFCC analyses for that column (zeros where no
 * frame precedes it).  processFrame runs TEN iterations there whatever the client's `iterations` parameter says (:113-116);
 * seed >= 0: every frame starts from the same K draws (a fresh generator of the seed per call), seed < 0: random_device.
 *
 * fluhip_nmffilter_f32 -- the audio outputs of NMFFilter: out[channel][component][n].  Per frame: processFrame (`iters`
 * iterations), the estimate W^T h as the ratio mask's denominator, component i's rank-one estimate through the mask
 * (exponent 1), inverse transform, window, overlap-add, division by the overlap-added squared window; the ring buffers'
 * delay of one window is removed as the wrapper removes it (frame m = 1, 2, ... covers samples [m hop - win, m hop)).
 * hop <= win. */
int fluhip_nmfmatch_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft, int64_t hop,
                        const float* bases, int64_t K, int64_t seed, int padding_mode, float* out, int64_t* frames_out);
int fluhip_nmffilter_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft, int64_t hop,
                         const float* bases, int64_t K, int64_t iters, int64_t seed, float* out);

/* ---- corpus: many independent equal-shape buffers, resident in HBM --------------------- */
/* The data-parallel form of the same path (BASELINE config 4): `count` mono buffers of n
 * samples each; every buffer is an independent BufNMF job (clients/nrt/NMFClient.hpp:233 loop
 * body; no cross-buffer state).  Lifetime: create -> set_audio -> stft -> nmf -> read-back. */
int  fluhip_corpus_create(fluhip_ctx* ctx, int64_t count, int64_t n, int64_t win, int64_t fft,
                          int64_t hop, int64_t K, fluhip_corpus** out);
void fluhip_corpus_destroy(fluhip_corpus* c);
int64_t fluhip_corpus_frames(const fluhip_corpus* c);   /* T */
int64_t fluhip_corpus_bins(const fluhip_corpus* c);     /* F */
int64_t fluhip_corpus_device_bytes(const fluhip_corpus* c);
/* audio: count x n floats, host (synchronous copy) or device pointer */
int fluhip_corpus_set_audio_host(fluhip_corpus* c, const float* audio);
int fluhip_corpus_set_audio_dev(fluhip_corpus* c, const float* audio_dev);
/* K1: batched window + real FFT + magnitude for every frame of every buffer */
int fluhip_corpus_stft(fluhip_corpus* c);
/* The same transform with the frame-major magnitudes ALONE -- STFT::process + STFT::magnitude of every buffer (alg/STFT.hpp:
 * 90-108, 61-66), no bin-major copy for the H update: what the spectrogram-only callers (fluhip_stft_*, BufSTFT) run, as a
 * corpus-sized batch.  fluhip_corpus_nmf then needs fluhip_corpus_stft again. */
int fluhip_corpus_stft_mag_only(fluhip_corpus* c);
/* NMF on every buffer; seeds: `count` seeds or NULL (then `seed` for all, like one ParameterSet
 * shared by all jobs).  Asynchronous on the context stream unless a progress callback is
 * given (progress is then reported per iteration across the whole batch). */
int fluhip_corpus_nmf(fluhip_corpus* c, int64_t iters, int update_w, int update_h, int64_t seed,
                      const int64_t* seeds, fluhip_progress_fn progress, void* user);
/* Seed / Fixed factors of the batched form: basesMode / actMode of clients/nrt/NMFClient.hpp:246-258 as they reach
 * NMF::process (alg/NMF.hpp:102-124: a given W0 / H0 replaces the random draw; clamping and normalisation :150-153 run
 * either way).  bases_seed: count x K x F floats or NULL; acts_seed: count x K x T floats or NULL -- channel-major per
 * buffer like BufferAdaptor::samps(component), the layout of fluhip_bufnmf_channel_f32's seeds.  The arrays are copied;
 * they apply to every later fluhip_corpus_nmf of this corpus until replaced (NULL: back to random draws from the seed).
 * Seed mode = seeds + update flag 1, Fixed mode = seeds + update flag 0 (fluhip_corpus_nmf's update_w / update_h). */
int fluhip_corpus_set_factors(fluhip_corpus* c, const float* bases_seed, const float* acts_seed);
/* RAGGED corpus: `count` mono buffers of DIFFERENT lengths n[i] (a folder of sound files) as one device-resident batch --
 * one STFT launch and one set of factor-update launches per iteration over all of them, the work dealt per wavefront
 * by each buffer's own frame count T_i = (n[i] + hop) / hop (long contractions are split, the strips of the H update
 * follow the buffer's frames).  Every buffer is the same independent BufNMF job as in an equal-length corpus
 * (clients/nrt/NMFClient.hpp:233 loop body).  Supported: ranks up to 128, fft 1024 / 2048 / 4096 with an even window
 * (FLUHIP_ERROR with a message otherwise: run such buffers as equal-length groups).  The other corpus entry points work
 * on a ragged corpus with T (n) = the longest buffer's frame (sample) count as the stride of every per-buffer array:
 * fluhip_corpus_stft, fluhip_corpus_nmf (seed / seeds), fluhip_corpus_set_factors (acts_seed: count x K x T, the entries
 * past a buffer's own frames are ignored), fluhip_corpus_read_f64 (frames past a buffer's own are zero),
 * fluhip_corpus_keep_spectrum + fluhip_corpus_resynth_dev (count x K x n, samples past a buffer's own untouched),
 * fluhip_corpus_plan. */
int fluhip_corpus_create_ragged(fluhip_ctx* ctx, int64_t count, const int64_t* n, int64_t win, int64_t fft, int64_t hop,
                                int64_t K, fluhip_corpus** out);
int64_t fluhip_corpus_frames_of(const fluhip_corpus* c, int64_t i);   /* T_i (T for an equal-length corpus) */
/* audio[i]: n[i] host floats */
int fluhip_corpus_set_audio_ragged_host(fluhip_corpus* c, const float* const* audio);
/* bases[i]: K x F floats, acts[i]: K x T_i floats (either array, or single entries, may be NULL) */
int fluhip_corpus_writeback_ragged_host(fluhip_corpus* c, float* const* bases, float* const* acts);
/* out[i]: K x n[i] floats (entries may be NULL): the resynthesised components of every buffer (see fluhip_corpus_resynth_dev) */
int fluhip_corpus_resynth_ragged_host(fluhip_corpus* c, float* const* out);
/* write-back (clients/nrt/NMFClient.hpp:277-300) into device or host float arrays:
 * bases: count x K x F, acts: count x K x T.  Either may be NULL. */
int fluhip_corpus_writeback_dev(fluhip_corpus* c, float* bases_dev, float* acts_dev);
int fluhip_corpus_writeback_host(fluhip_corpus* c, float* bases, float* acts);
/* Resynthesis of every component of every buffer (clients/nrt/NMFClient.hpp:302-334: NMF::estimate -> RatioMask ->
 * ISTFT): out = count x K x n floats.  The complex spectrogram has to be kept for it: switch that on before
 * fluhip_corpus_stft (it costs count x T x F x 16 bytes of HBM). */
int fluhip_corpus_keep_spectrum(fluhip_corpus* c, int on);
int fluhip_corpus_resynth_dev(fluhip_corpus* c, float* out_dev);
int fluhip_corpus_resynth_host(fluhip_corpus* c, float* out);
/* The resynthesis written the way an interleaved host buffer holds it (frames x channels, like MemoryBufferAdaptor,
 * clients/common/MemoryBufferAdaptor.hpp:96-100): out[t * frame_stride + b * K + k] = component k of buffer b at sample t,
 * i.e. what resynth.samps(b * rank + k) <<= ... leaves there (clients/nrt/NMFClient.hpp:321-326), transposed on the device
 * and streamed to the host through pinned staging blocks.  frame_stride >= count x K floats; equal-length corpora only. */
int fluhip_corpus_resynth_interleaved_host(fluhip_corpus* c, float* out, int64_t frame_stride);
/* raw f64 results for parity tests: mag count x T x F, W1 count x K x F, H1 count x T x K */
int fluhip_corpus_read_f64(fluhip_corpus* c, double* mag, double* W1, double* H1);
/* Diagnostic for parity tests: the corpus's spectrogram layouts AS THEY LIE on the device, padding included.  dims5 (may be
 * NULL) = { count, Fp, Tp, T, F } (Fp, Tp: bins and frames rounded up to 32, the leading dimensions); with every array NULL
 * the call only reports them.  mag: count x Tp x Fp frame-major magnitudes (also after fluhip_corpus_stft_mag_only, where
 * fluhip_corpus_read_f64 has no spectrogram to report); magT: count x Fp x Tp, the bin-major copy the H update streams
 * (fluhip_corpus_stft only; columns T .. Tp and the frames past a ragged buffer's own are zero); spec: count x T x F x 2,
 * the complex spectrum kept under fluhip_corpus_keep_spectrum (rows past a ragged buffer's own frames are not written). */
int fluhip_debug_corpus_read_layouts_f64(fluhip_corpus* c, int64_t* dims5, double* mag, double* magT, double* spec);
/* How the factor updates of this corpus are scheduled on the device (introspection for tests, benchmarks and
 * bug reports; no effect on results beyond summation order): out8 = { kernel form (5 = 4x4x4 MFMA + LDS-DMA, ranks up to
 * 128; 0 = the un-fused any-rank path above that), contraction splits of the W update, of the H update (low 16 bits;
 * bits 16.. = the pieces of the tail launch when the H update goes out as two launches, 0 otherwise),
 * deferred column normalisation of W (alg/NMF.hpp:162 applied on load) 0/1, Nyquist bin as a side column 0/1,
 * wavefronts per buffer of the W update, padded rank (low 16 bits: the rank the arrays are laid out for -- 16, 32, 64, 128;
 * bits 16..: the rank the factor updates COMPUTE -- 24 for ranks 17 .. 24; 40 / 48 / 56 for 33 .. 40 / 48 / 56; 72, 80 .. 112 for 65 .. 72, .. 80, .. 112; else the padded rank),
 * frame-strip schedule 0/1 (a single buffer of rank <= 16: the H
 * update local to a strip of frames, the W update's numerator as per-workgroup partials + a reduce launch; the split
 * counts before it then describe the schedule it replaces) }. */
int fluhip_corpus_plan(const fluhip_corpus* c, int64_t* out8);

/* Introspection for the tests (pure host code, no device needed): the work lists the planner builds for `count` buffers of
 * frames[i] frames and `bins` bins at rank K -- which = 0 the W update's, 1 the H update's.  desc (may be NULL) receives up to
 * `cap` descriptors of 12 ints {buffer, first column group, groups, first step, end step, partial slot, statistics slot,
 * denominator slot, group word (leader | rank << 4 | size << 8 | barrier << 16), 0, 0, 0}, four per workgroup; info8 =
 * {workgroups, widest strip, partials in memory 0/1, most partials per buffer, most pieces per contraction, partial slots,
 * Nyquist side column 0/1, statistics parts per buffer}.  Returns the number of descriptors (-1: bad arguments). */
int64_t fluhip_debug_plan_lists(int64_t count, const int64_t* frames, int64_t bins, int64_t K, int which, int32_t* desc,
                                int64_t cap, int32_t* info8);

/* Likewise for the two-launch form of the H update (corpus_plan.hip plan_tail): `count` equal-length buffers of `frames` frames and
 * `bins` bins at rank K.  out4 = {pieces of the tail launch's contraction (0: the update stays one launch), strips per buffer
 * of the first launch, strips per buffer of the tail launch, frames per buffer in the first launch}. */
int fluhip_debug_plan_tail(int64_t count, int64_t frames, int64_t bins, int64_t K, int64_t* out4);
/* Which schedule family an equal-length corpus of that shape gets when nothing else decides first (a single buffer of rank <= 16
 * that fits the frame-strip schedule never asks): 1 = the work lists, 0 = the uniform schedule; -1: bad arguments.  The rules are
 * measured ones (corpus_plan.hip list_plan_pays, profiles/r03/plan_regimes.txt); the CPU tests pin them for the BASELINE shapes. */
int fluhip_debug_plan_kind(int64_t count, int64_t frames, int64_t bins, int64_t K);
/* What the H update of an equal-length corpus of that shape takes over from the launches that used to run between the two
 * factor updates (kernels_nmf5.hip SIDEQ forms; no device needed): bit 0 = the next W update's side column (its last bin)
 * comes out of this launch's epilogue, bit 1 = the norm combine of the W update in front is done in its prologue; 0 = neither
 * (rank above 64, work lists, two-launch H update, no side column at this bin count); -1: bad arguments. */
int fluhip_debug_plan_h_update(int64_t count, int64_t frames, int64_t bins, int64_t K);
/* The WHOLE schedule of an equal-length corpus of that shape as data, without a device (corpus_plan.hip decide_update_plan: the
 * one function fluhip_corpus_create plans from).  out32 =
 *   0 kernel family (5 / 0)   1 pieces of the W update's contraction   2 of the H update's   3 deferred normalisation
 *   4 Nyquist bin as a side column   5 statistics records per buffer of a W update   6 padded rank   7 computed rank
 *   8 frame-strip schedule (0 no, 1 fused, 2 / 3 the A/B forms)   9 work lists   10 pieces of the tail launch of a two-launch H
 *   update (0: one launch)   11 strips of its first launch   12 of its tail launch   13 frames in the first launch
 *   14 wavefronts per buffer of a uniform H update
 *   15 .. 21 workspaces in doubles, as allocated: split partials, denominators, column-sum pre-pass, norm / side-column scratch,
 *            column partials of the W update, frame-strip partials, any-rank scratch
 *   22 what the H update takes over in the steady state (bit 0 side column, bit 1 norm combine, bit 2 column sums from the W update)
 *   23 form of the norm-combine launch between the updates (fluhip_debug_wnorm_form's codes; -1: no such launch)
 *   24 slices of the side-column launch (0: none)   25 side-partial slots per buffer and generation   26 doubles of wscratch the
 *      statistics records occupy.
 * tests/test_plan_table.py holds this to its invariants over a grid of shapes and to the pinned plans of the BASELINE shapes. */
int fluhip_debug_plan_shape(int64_t count, int64_t frames, int64_t bins, int64_t K, int64_t* out32);
/* the form the norm combine of a W update takes (kernels_nmf.hip kWnormForms, the one table of its thresholds): 0 side column +
 * combine in one launch, 1 side-column launch only, 2 pre-reduction + combine, 3 one workgroup of 1024 threads, 4 of 256 */
int fluhip_debug_wnorm_form(int Kp, int count, int parts, int slices, int side_rows, int side_phase, int want_colsum);

/* ---- device pool: one host process, several GPUs ------------------------------------------------------------ */
/* The reference runs one std::thread per job (clients/common/FluidNRTClientWrapper.hpp:1042-1048) and the buffers of
 * a corpus are independent jobs (clients/nrt/NMFClient.hpp:233 loop body): a pool holds one context per listed device
 * and, per call, one host thread per device; buffers are dealt in contiguous blocks (fluhip_shard_range, remainder
 * over the first members) and every device writes its share of the result straight into the caller's arrays.
 * devices == NULL: every visible device.  A device may be listed more than once (two contexts on one GPU).
 * Multi-PROCESS jobs (one rank per GPU) use the same dealing and gather with RCCL: flucoma-core_amd/sharding.py. */
typedef struct fluhip_pool fluhip_pool;
int         fluhip_pool_create(const int* devices, int n_devices, fluhip_pool** out);
void        fluhip_pool_destroy(fluhip_pool* pool);
int         fluhip_pool_size(const fluhip_pool* pool);
int         fluhip_pool_device(const fluhip_pool* pool, int member);
const char* fluhip_pool_last_error(const fluhip_pool* pool);
/* BufNMF over `count` equal-length mono buffers (BASELINE config 4): audio count x n host floats; bases count x K x F,
 * acts count x K x T host floats (either may be NULL); seeds: `count` seeds or NULL.  progress (may be NULL) is called
 * on the calling thread with iteration = 1..iters in order, an iteration counting once every device has passed it;
 * returning 0 cancels every device's share (FLUHIP_CANCELLED). */
int fluhip_pool_bufnmf_f32(fluhip_pool* pool, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft,
                           int64_t hop, int64_t K, int64_t iters, int update_w, int update_h, int64_t seed,
                           const int64_t* seeds, float* bases, float* acts, fluhip_progress_fn progress, void* user);
/* The whole BufNMF parameter set of the batched form in one description: Seed / Fixed factors (basesMode / actMode,
 * clients/nrt/NMFClient.hpp:63-67, 246-258) and the resynthesis output (resynthMode 1, :302-334) on top of what
 * fluhip_pool_bufnmf_f32 takes.  Zero-initialise, then fill in what the job uses. */
typedef struct fluhip_bufnmf_job
{
  int64_t count, n;                  /* equal-length mono buffers, samples each */
  int64_t win, fft, hop, K, iters;
  int     update_w, update_h;        /* 0 together with the matching seed array = Fixed mode */
  int64_t seed;                      /* randomSeed for every buffer ... */
  const int64_t* seeds;              /* ... or `count` seeds (NULL: `seed`) */
  const float* audio;                /* count x n */
  const float* bases_seed;           /* count x K x F or NULL */
  const float* acts_seed;            /* count x K x T or NULL */
  float* bases;                      /* count x K x F or NULL */
  float* acts;                       /* count x K x T or NULL */
  float* resynth;                    /* count x K x n or NULL */
} fluhip_bufnmf_job;
int fluhip_pool_bufnmf_job_f32(fluhip_pool* pool, const fluhip_bufnmf_job* job, fluhip_progress_fn progress, void* user);
/* The same over buffers of DIFFERENT lengths (a folder of sound files): audio[i] = n[i] host floats; bases[i] receives
 * K x F, acts[i] K x T_i floats with T_i = fluhip_stft_num_frames(n[i], win, hop) (either array, or single entries, may be
 * NULL).  Buffers are dealt by fluhip_balanced_assignment over their frame counts; a device's share runs as ONE ragged
 * corpus (all its buffers advance together, iteration by iteration); shapes the ragged form does not cover are
 * processed run by run of equal length.  progress (may be NULL) is called on the calling thread with the number of
 * buffers finished so far, ascending up to count -- in the ragged form a device's whole share finishes at once, so the
 * count moves in steps of a share, not buffer by buffer; returning 0 stops every device at its next iteration
 * (FLUHIP_CANCELLED; the outputs of unfinished buffers are not written).  Without a callback the iterations are
 * enqueued without the per-iteration host round trip a cancellable job needs. */
int fluhip_pool_bufnmf_ragged_f32(fluhip_pool* pool, const float* const* audio, const int64_t* n, int64_t count, int64_t win,
                                  int64_t fft, int64_t hop, int64_t K, int64_t iters, int update_w, int update_h, int64_t seed,
                                  const int64_t* seeds, float* const* bases, float* const* acts, fluhip_progress_fn progress,
                                  void* user);
/* The feature pipeline over the pool (BASELINE config 5, "1 -> 8 GPU scaling"): `count` equal-length slices, dealt in
 * contiguous blocks; audio: count x n host floats, out: count x nFeatures x T host floats (see fluhip_bufmfcc_padded_f32 /
 * fluhip_bufmelbands_padded_f32 for the arguments).  The slices are independent analyses: no exchange between devices. */
int fluhip_pool_bufmfcc_f32(fluhip_pool* pool, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft,
                            int64_t hop, int64_t n_bands, int64_t n_coefs, int64_t start_coeff, double min_freq,
                            double max_freq, double sample_rate, int padding_mode, float* out, int64_t* frames_out);
int fluhip_pool_bufmelbands_f32(fluhip_pool* pool, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft,
                                int64_t hop, int64_t n_bands, double min_freq, double max_freq, double sample_rate,
                                int normalize, int scale_db, int padding_mode, float* out, int64_t* frames_out);

/* the dealing itself (integer arithmetic, also used by the multi-process launcher): contiguous blocks [begin, end) of
 * n_items over `world` ranks; and the greedy longest-processing-time deal for ragged corpora (cost ~ T F K per buffer,
 * ties to the lower index / rank): rank_of_item[i] = rank of item i */
void fluhip_shard_range(int64_t n_items, int world, int rank, int64_t* begin, int64_t* end);
int  fluhip_balanced_assignment(const double* costs, int64_t n, int world, int32_t* rank_of_item);

/* ---- live kernel timing (HIP events on the context stream) ----------------------------- */
/* When enabled, every launch of the two dominant kernel classes is bracketed by hipEvents on
 * the stream it is launched on.  Classes: 0 = the STFT kernel (both magnitude layouts), 1 = nmf_update (both factor
 * updates share one kernel; the split-contraction finalize counts with it), 2 = feature kernels, 3 = the small kernels
 * between the factor updates, 4 = the transposing copy of shapes the block STFT kernel does not cover, 5 = the mask kernel of
 * BufHPSS, 6 = its inverse transforms (one record per round of buffers).  fluhip_prof_read synchronises and returns the launch count and the summed duration
 * since the last reset. */
int fluhip_prof_enable(fluhip_ctx* ctx, int on);
int fluhip_prof_reset(fluhip_ctx* ctx);
int fluhip_prof_read(fluhip_ctx* ctx, int kernel_class, int64_t* launches, double* total_ms);
/* Box-invariant cost of the factor-update launches of a corpus (kernels_nmf5.hip): one wavefront per launch -- it lives as
 * long as the launch does -- adds its shader cycles (s_memtime) and 100 MHz ticks (s_memrealtime) to a device record.
 * out8 = { W update: launches, shader cycles, 100 MHz ticks, 0;  H update: the same four }.  cycles / launches is what a
 * kernel change moves whatever clock the box sustains; cycles / ticks * 100 MHz is that sustained clock.  Zero counts when
 * the corpus runs a schedule without the stamps (frame-strip schedule, A/B kernel forms).  reset != 0 clears the record. */
int fluhip_corpus_update_clocks(fluhip_corpus* c, int64_t* out8, int reset);
/* Device time of the last fluhip_corpus_nmf iteration loop of this corpus: two HIP events on the context stream, the first
 * recorded BEHIND the host-side initialisation (random draws, uploads), the second behind the loop's last launch (the
 * deferred-normalisation apply excluded).  Synchronises on the second event.  What tools/perf_matrix.py divides by the
 * iteration count: no host scheduling, no initialisation inside the figure. */
int fluhip_corpus_last_loop_ms(fluhip_corpus* c, double* ms);
/* Kernel-developer diagnostic: with FLUHIP_K5_INSTR=1 in the environment the factor-update kernel of the
 * c4-shaped schedules runs an instrumented build that leaves cycle counters and a timeline of one wavefront in the
 * corpus' scratch; this copies the first 32 words out (tools/phase_breakdown.py decodes them).  Without the
 * environment variable the words are whatever the scratch holds. */
int fluhip_corpus_debug_words(fluhip_corpus* c, int64_t* out32);

#ifdef __cplusplus
}
#endif
#endif /* FLUCOMA_HIP_H */
