/* flamo_hip_melmss.h -- C ABI of the mel multi-scale spectral criterion (csrc/melmss.hip), the seventh header of
 * libflamo_hip.so.
 *
 * Same conventions as flamo_hip.h (which declares the error codes and fl_last_error): every fl_*_f32 / _f64 function returns
 * FL_OK or an FL_ERR_* code, pointers are device addresses unless said otherwise, `stream` is a hipStream_t, nothing
 * synchronises with the host and nothing allocates.  One declaration per `;`, every parameter named: flamo_amd/_lib.py reads
 * the ctypes signatures from this text.
 *
 * The criterion compares a prediction and a target of shape (B, T, N); element (b, t, c) of the prediction is at
 * yp[b * spb + t * spt + c * spc] and of the target at yt[b * stb + t * stt + c * stc] (element strides of any sign, nothing
 * is copied).  Every (b, c) column is one row, B N rows.  `res` is a HOST array of R triples (n_fft, hop, nnz), one per
 * resolution; for each of them
 *   frames   F = 1 + T / hop frames of n_fft samples of the row reflect-padded by n_fft / 2 on each side, each multiplied by
 *            the window of n_fft samples;  X[k] its transform, k = 0 .. n_fft / 2
 *   P        re^2 + im^2 (its gradient at an exact zero is 0)
 *   m        W P, W the (n_fft / 8, n_fft / 2 + 1) mel basis: n_fft / 8 band energies per frame
 *   mask     1, or with apply_mask 0 where 10 log10(max(m_t^2, 1.01 ne) - ne) - 10 log10(ne) < threshold, ne = noise_energy;
 *            it depends on the target alone
 *   Nn       the number of entries of m_t (rows x bands x frames), or with apply_mask the sum of the mask
 *   term     |(m_t - m_p) mask| / Nn, and with log_term also alpha |(log m_t - log m_p) mask| / Nn; |.| is the square root
 *            of the sum of squares over everything at once (norm = 2) or the sum of absolute values (norm = 1)
 * and the loss is the SUM of the terms over the resolutions.  Nothing is clamped: a band that is exactly 0 in either signal
 * makes the log term non-finite, and Nn = 0 divides as IEEE does.  The gradient of a norm = 2 term whose sum of squares is 0
 * is 0; the sign of a difference that is 0 is 0.
 * Sizes the kernels take: 1 <= R <= 8, n_fft a power of two from 128 to 4096, hop >= 1, n_fft / 2 < T <= 2^30, B, N >= 1,
 * fewer than 2^31 frames and at most 2^38 samples in all, 0 <= nnz <= (n_fft / 8) (n_fft / 2 + 1), norm 1 or 2, and with
 * apply_mask a noise_energy > 0.
 * wtab holds the windows of the resolutions one behind the other (n_fft DOUBLES each, in float32 too); tw[j] =
 * exp(-2 pi i j / 4096), j < 4096, is the complex DOUBLE table of fl_twiddle_fill_f64 for length 4096: both precisions
 * transform in double, and only the signals, gframes, gy, loss and gloss have the signals' type.
 * The mel bases are the caller's host matrices, handed over as two tables in the format of flamo_hip_edr.h with n_fft / 8 in
 * the place of 64, those of the resolutions one behind the other.  melidx (fl_melmss_mel_ints int32), per resolution:
 * start[n_fft / 8], count[n_fft / 8], offset[n_fft / 8] -- band j holds the bins start[j] .. start[j] + count[j] - 1, their
 * weights at this resolution's melw[offset[j] ..] -- then band[n_fft / 2 + 1]: bin k lies in the bands band[k] and band[k] + 1
 * and no other.  melw (fl_melmss_mel_doubles doubles), per resolution: the nnz packed weights, then for every bin k its
 * weights in band[k] and in band[k] + 1.  The kernels clamp what they read from melidx to the arrays it indexes.
 *
 *   fl_melmss_frames        B N (F_0 + ... + F_{R-1}), or -1 for sizes the kernels do not take (the support query); `partial`
 *                           holds 5 doubles per frame
 *   fl_melmss_gframe_elems  elements of `gframes` (the sum of B N F n_fft), or -1
 *   fl_melmss_keep_doubles  doubles of `keep` (65): per resolution the five sums and the two factors of dL/dm_p, then the loss
 *   fl_melmss_mel_ints      ints of melidx, or -1
 *   fl_melmss_mel_doubles   doubles of melw, or -1
 *   fl_melmss_launches      the kernel launches of fl_melmss_fwd (backward = 0) or fl_melmss_bwd (backward = 1) for these
 *                           resolutions, or -1: it depends on the list of n_fft alone, never on B, T, N or the data
 *   fl_melmss_fwd_*         at most FOUR launches: the frame kernel of the resolutions with n_fft <= 1024 (one wavefront per
 *                           (resolution, row, frame)), the frame kernel of those with n_fft > 1024 (one workgroup of four
 *                           wavefronts per (resolution, row, frame)) -- windowed reflect-indexed loads of prediction and
 *                           target, two real transforms, |X|^2 in LDS, the band sums taken from there, five doubles per frame
 *                           into `partial` (sum mask d^2, sum mask |d|, the same two of the log difference, sum mask) -- the
 *                           combine (one workgroup per resolution, a fixed order) and the final kernel, which writes keep
 *                           and loss[0].  A size class without a resolution is not launched.
 *   fl_melmss_bwd_*         at most THREE launches: the two frame kernels (both transforms recomputed, dL/dm_p formed, dL/dP
 *                           gathered from the two bands of a bin, dL/dX = 2 X dL/dP, the adjoint of the real-transform split,
 *                           the inverse transform; the n_fft samples of a frame go to gframes) and the overlap-add, a gather
 *                           per sample in a fixed order with the reflected margins folded back: gy (contiguous (B, T, N)) =
 *                           gloss[0] times the gradient of the loss.
 * loss and gloss are device scalars of the signals' type; partial and keep device doubles.  Every sum is taken in a fixed
 * order (no atomics); everything behind the loads of the signals is a double in both precisions. */
#ifndef FLAMO_HIP_MELMSS_H
#define FLAMO_HIP_MELMSS_H

#ifdef __cplusplus
extern "C" {
#endif

long fl_melmss_frames(long B, long T, long N, int R, int* res);
long fl_melmss_gframe_elems(long B, long T, long N, int R, int* res);
long fl_melmss_keep_doubles(void);
long fl_melmss_mel_ints(int R, int* res);
long fl_melmss_mel_doubles(int R, int* res);
long fl_melmss_launches(int R, int* res, int backward);

int fl_melmss_fwd_f32(const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long T,
                      long N, int R, int* res, const void* wtab, const void* tw, const void* melidx, const void* melw, int norm,
                      int log_term, double alpha, int apply_mask, double threshold, double noise_energy, void* partial,
                      void* keep, void* loss, void* stream);
int fl_melmss_fwd_f64(const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long T,
                      long N, int R, int* res, const void* wtab, const void* tw, const void* melidx, const void* melw, int norm,
                      int log_term, double alpha, int apply_mask, double threshold, double noise_energy, void* partial,
                      void* keep, void* loss, void* stream);

int fl_melmss_bwd_f32(const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long T,
                      long N, int R, int* res, const void* wtab, const void* tw, const void* melidx, const void* melw, int norm,
                      int log_term, int apply_mask, double threshold, double noise_energy, const void* keep, const void* gloss,
                      void* gframes, void* gy, void* stream);
int fl_melmss_bwd_f64(const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long T,
                      long N, int R, int* res, const void* wtab, const void* tw, const void* melidx, const void* melw, int norm,
                      int log_term, int apply_mask, double threshold, double noise_energy, const void* keep, const void* gloss,
                      void* gframes, void* gy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLAMO_HIP_MELMSS_H */
