/* flamo_hip_mss.h -- C ABI of the linear multi-scale spectral criterion (csrc/mss.hip), the ninth header of libflamo_hip.so.
 *
 * Same conventions as flamo_hip.h (which declares the error codes and fl_last_error): every fl_*_f32 / _f64 function returns
 * FL_OK or an FL_ERR_* code, pointers are device addresses unless said otherwise, `stream` is a hipStream_t, nothing
 * synchronises with the host and nothing allocates.  One declaration per `;`, every parameter named: flamo_amd/_lib.py reads
 * the ctypes signatures from this text.
 *
 * The criterion compares a prediction and a target of shape (B, T, N); element (b, t, c) of the prediction is at
 * yp[b * spb + t * spt + c * spc] and of the target at yt[b * stb + t * stt + c * stc] (element strides of any sign, nothing
 * is copied).  Every (b, c) column is one row, B N rows.  `res` is a HOST array of R pairs (n_fft, hop), one per resolution;
 * for each of them, with n = n_fft and K = n / 2 + 1,
 *   frames   F = 1 + T / hop frames of n samples of the row reflect-padded by n / 2 on each side, each multiplied by the
 *            window w of n samples
 *   X[k, f]  sum_{j < n} w_j x[f hop + j] exp(-2 pi i beta_k j / n), k < K: a framed DFT at the equispaced but fractional bin
 *            positions beta_k = a + k s (a zoom transform; the caller's tables hold the basis, see below)
 *   M        sqrt(re^2 + im^2); its gradient at an exact zero is 0
 *   mask     1, or with apply_mask 0 where 10 log10(max(M_t^2, 1.01 ne) - ne) - 10 log10(ne) < threshold, ne = noise_energy;
 *            it depends on the target alone
 *   d, dl    (M_t - M_p) mask and (log M_t - log M_p) mask
 *   term     form 0: |d| / Nn, and with log_term also alpha |dl| / Nn; |.| is the square root of the sum of squares over
 *                    everything at once (norm = 2) or the sum of absolute values (norm = 1); Nn the number of entries of M_t
 *                    (rows x K x F), or with apply_mask the sum of the mask
 *            form 1: |d|_2 / |M_t|_2 + alpha |dl|_1 / numel(M_t)        ("yamamoto": the denominator is not masked; norm and
 *                    log_term are ignored)
 *            form 2: (|d|_1 + alpha |dl|_1) / numel(M_t)                ("magenta")
 * and the loss is the SUM of the terms over the resolutions.  Nothing is clamped: a bin that is exactly 0 in either signal
 * makes a log term non-finite, and a zero denominator divides as IEEE does.  The gradient of a 2-norm whose sum of squares is
 * 0 is 0; the sign of a difference that is 0 is 0.
 * Sizes the kernels take: 1 <= R <= 8, n_fft a multiple of 4 from 16 to 4096 (no power of two is asked for), hop >= 1,
 * n_fft / 2 < T <= 2^30, B, N >= 1, fewer than 2^31 frames, fewer than 2^24 workgroups in either tile grid and fewer than
 * 2^32 samples in all (no launch reaches 2^32 threads), norm 1 or 2, form 0, 1 or 2, and
 * with apply_mask a finite noise_energy > 0.
 *
 * `tab` (fl_mss_table_doubles DOUBLES, in float32 too, aligned to 16 bytes) holds per resolution, one behind the other, with
 * theta_k = 2 pi beta_k / n, NJ = ceil(n / 64) and NK = ceil(K / 64):
 *   w        n doubles, the window
 *   fseed    K NJ complex, fseed[k NJ + m] = exp(-i theta_k 64 m)
 *   fstep    K 5 complex,  fstep[k 5 + c]  = exp(-i theta_k c), c = 0 .. 4
 *   bseed    n NK complex, bseed[j NK + m] = exp(+i theta_{64 m} j)
 *   bstep    n 5 complex,  bstep[j 5 + c]  = exp(+i (theta_c - theta_0) j), c = 0 .. 4
 * The basis itself is never stored: a lane of the forward kernel starts a run of 64 samples at fseed fstep[lane's offset] and
 * advances by fstep[4], sixteen times; the adjoint kernel does the same along the bins with bseed and bstep.
 *
 *   fl_mss_frames          B N (F_0 + ... + F_{R-1}), or -1 for sizes the kernels do not take (the support query)
 *   fl_mss_partial_doubles doubles of `partial` (6 per workgroup of the tile kernel), or -1
 *   fl_mss_keep_doubles    doubles of `keep`, or -1: 65 (per resolution the six sums and the two factors of dL/dM_p, then the
 *                          loss) and, with planes != 0, three planes of B N F K doubles per resolution behind them -- the
 *                          prediction's X (re, im) and the target's M, laid out (row, frame, bin)
 *   fl_mss_gframe_elems    elements of `gframes` (the sum of B N F n_fft), or -1
 *   fl_mss_table_doubles   doubles of `tab`, or -1
 *   fl_mss_launches        the kernel launches of fl_mss_fwd (backward = 0) or fl_mss_bwd (backward = 1) for these
 *                          resolutions, or -1: 3 and 2, whatever the list, B, T, N and the data
 *   fl_mss_fwd_*           THREE launches.  The tile kernel: one workgroup of four wavefronts per (resolution, row, 16 frames,
 *                          256 bins), the longest resolutions first; the windowed frames are staged in LDS 64 samples at a
 *                          time, each wavefront holds 4 tiles of 16 frames x 16 bins as real and imaginary accumulators of
 *                          v_mfma_f64_16x16x4_f64 and generates its basis columns by rotation; prediction and target run
 *                          through one loop body.  With planes != 0 the prediction's X and the target's M go to keep.  Six
 *                          doubles per workgroup go to `partial` (sum mask d^2, sum mask |d|, the same two of dl, sum mask,
 *                          sum M_t^2).  Then the combine (one workgroup per resolution, a fixed order) and the final kernel,
 *                          which writes the head of keep and loss[0].
 *   fl_mss_bwd_*           TWO launches.  The adjoint tile kernel: one workgroup per (resolution, row, 16 frames, 512 samples
 *                          of the frame); G = dL/dM_p X_p / M_p (0 where M_p is 0) is formed from the kept planes 64 bins at a
 *                          time in LDS, gframe[f, j] = w_j sum_k Re(G[k, f] exp(+i theta_k j)) on the same matrix
 *                          instruction, the n_fft samples of a frame go to gframes.  Then the overlap-add, a gather per
 *                          sample in a fixed order with the reflected margins folded back: gy (contiguous (B, T, N)) =
 *                          gloss[0] times the gradient of the loss.  keep must be that of a forward call with planes != 0.
 * loss and gloss are device scalars of the signals' type; partial, keep and tab device doubles.  Every sum is taken in a fixed
 * order (no atomics); everything between the loads of the signals and the stores of gframes is a double in both precisions. */
#ifndef FLAMO_HIP_MSS_H
#define FLAMO_HIP_MSS_H

#ifdef __cplusplus
extern "C" {
#endif

long fl_mss_frames(long B, long T, long N, int R, int* res);
long fl_mss_partial_doubles(long B, long T, long N, int R, int* res);
long fl_mss_keep_doubles(long B, long T, long N, int R, int* res, int planes);
long fl_mss_gframe_elems(long B, long T, long N, int R, int* res);
long fl_mss_table_doubles(int R, int* res);
long fl_mss_launches(int R, int* res, int backward);

int fl_mss_fwd_f32(const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long T,
                   long N, int R, int* res, const void* tab, int norm, int form, int log_term, double alpha, int apply_mask,
                   double threshold, double noise_energy, int planes, void* partial, void* keep, void* loss, void* stream);
int fl_mss_fwd_f64(const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long T,
                   long N, int R, int* res, const void* tab, int norm, int form, int log_term, double alpha, int apply_mask,
                   double threshold, double noise_energy, int planes, void* partial, void* keep, void* loss, void* stream);

int fl_mss_bwd_f32(long B, long T, long N, int R, int* res, const void* tab, int norm, int form, int log_term, int apply_mask,
                   double threshold, double noise_energy, const void* keep, const void* gloss, void* gframes, void* gy,
                   void* stream);
int fl_mss_bwd_f64(long B, long T, long N, int R, int* res, const void* tab, int norm, int form, int log_term, int apply_mask,
                   double threshold, double noise_energy, const void* keep, const void* gloss, void* gframes, void* gy,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLAMO_HIP_MSS_H */
