/* flamo_hip_mrstft.h -- C ABI of the multi-resolution STFT criterion (csrc/mrstft.hip), the fifth header of libflamo_hip.so.
 *
 * Same conventions as flamo_hip.h (which declares the error codes and fl_last_error): every fl_*_f32 / _f64 function returns
 * FL_OK or an FL_ERR_* code, pointers are device addresses unless said otherwise, `stream` is a hipStream_t, nothing
 * synchronises with the host and nothing allocates.  One declaration per `;`, every parameter named: flamo_amd/_lib.py reads
 * the ctypes signatures from this text.
 *
 * The criterion compares a prediction and a target of shape (B, T, N); element (b, t, c) of the prediction is at
 * yp[b * spb + t * spt + c * spc] and of the target at yt[b * stb + t * stt + c * stc] (element strides of any sign, nothing
 * is copied).  Every (b, c) column is one row, B N rows.  `res` is a HOST array of 3 R ints, (n_fft, hop, win) per resolution.
 * For each resolution:
 *   frames   F = 1 + T / hop frames of n_fft samples of the row reflect-padded by n_fft / 2 on each side, each multiplied by
 *            the window of win samples centred in the frame (left pad (n_fft - win) / 2);  X[k] its transform, k = 0 .. n_fft/2
 *   M        sqrt(max(re^2 + im^2, eps)) of the prediction (M_p) and the target (M_t)
 *   sums     D = sum (M_t - M_p)^2,  S = sum M_t^2,  G = sum |log M_p - log M_t|,  A = sum |M_p - M_t| over rows, bins, frames
 *   loss     (1 / R) sum_r (w_sc sqrt(D_r) / sqrt(S_r) + w_log G_r / n_r + w_lin A_r / n_r),  n_r = B N F_r (n_fft_r / 2 + 1)
 * Sizes the kernels take: 1 <= R <= 8, n_fft a power of two from 256 to 2048, 1 <= win <= n_fft, hop >= 1,
 * n_fft / 2 < T <= 2^30, B, N >= 1, fewer than 2^31 frames and at most 2^38 samples in all.
 * wtab holds the windows of the resolutions one behind the other (win_0 + win_1 + ... DOUBLES, in float32 too);
 * tw[j] = exp(-2 pi i j / 2048), j < 2048, is the complex DOUBLE table of fl_twiddle_fill_f64 for length 2048: both precisions
 * transform in double, and only the signals, gframes, gy, loss and gloss have the signals' type.
 *
 *   fl_mrstft_blocks        frames of all resolutions and rows (one workgroup and four partial sums each), or -1 for sizes
 *                           the kernels do not take
 *   fl_mrstft_gframe_elems  elements of `gframes` (B N F_r win_r summed over the resolutions), or -1
 *   fl_mrstft_keep_doubles  doubles of `keep` (65): what the backward entry reads again -- keep[8 r + 0..3] = D, S, G, A of
 *                           resolution r, keep[8 r + 4..6] = the factors of dL/dM_p (of M_p - M_t, of sign / M_p, of sign),
 *                           keep[64] = the loss
 *   fl_mrstft_fwd_*         THREE launches for all resolutions, rows and both signals: the frame kernel (one wavefront per
 *                           frame: windowed reflect-indexed loads of prediction and target, two real transforms, the frame's
 *                           four sums in double into partial[4 * blocks]), the combine (one workgroup per resolution, fixed
 *                           order) and the final kernel, which writes keep and loss[0]
 *   fl_mrstft_bwd_*         TWO launches: the frame kernel again (both transforms recomputed, dL/dM_p from keep, the adjoint
 *                           of the real-transform split, the inverse transform; the win samples under the window go to
 *                           gframes) and the overlap-add, a gather per sample in a fixed order with the reflected margins
 *                           folded back: gy (contiguous (B, T, N)) = gloss[0] times the gradient of the loss.  The gradient
 *                           of M is 0 where re^2 + im^2 <= eps.
 * loss and gloss are device scalars of the signals' type, partial and keep device doubles.  Every sum is taken in a fixed
 * order (no atomics); everything behind the loads of the signals is a double in both precisions. */
#ifndef FLAMO_HIP_MRSTFT_H
#define FLAMO_HIP_MRSTFT_H

#ifdef __cplusplus
extern "C" {
#endif

long fl_mrstft_blocks(long B, long T, long N, int R, int* res);
long fl_mrstft_gframe_elems(long B, long T, long N, int R, int* res);
long fl_mrstft_keep_doubles(void);

int fl_mrstft_fwd_f32(const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long T,
                      long N, int R, int* res, const void* wtab, const void* tw, double w_sc, double w_log, double w_lin,
                      double eps, void* partial, void* keep, void* loss, void* stream);
int fl_mrstft_fwd_f64(const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long T,
                      long N, int R, int* res, const void* wtab, const void* tw, double w_sc, double w_log, double w_lin,
                      double eps, void* partial, void* keep, void* loss, void* stream);

int fl_mrstft_bwd_f32(const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long T,
                      long N, int R, int* res, const void* wtab, const void* tw, double eps, const void* keep,
                      const void* gloss, void* gframes, void* gy, void* stream);
int fl_mrstft_bwd_f64(const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long T,
                      long N, int R, int* res, const void* wtab, const void* tw, double eps, const void* keep,
                      const void* gloss, void* gframes, void* gy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLAMO_HIP_MRSTFT_H */
