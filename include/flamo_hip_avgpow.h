/* flamo_hip_avgpow.h -- C ABI of the average-power criterion (csrc/avgpow.hip), the third header of libflamo_hip.so.
 *
 * Same conventions as flamo_hip.h (which declares the error codes and fl_last_error): every fl_*_f32 / _f64 function returns
 * FL_OK or an FL_ERR_* code, pointers are device addresses, `stream` is a hipStream_t, nothing synchronises with the host and
 * nothing allocates.  One declaration per `;`, every parameter named: flamo_amd/_lib.py reads the ctypes signatures from
 * this text.
 *
 * The criterion (the reference's AveragePower, flamo/optimize/loss.py:462-549) compares two signals of T samples, sample t of
 * the prediction at yp[t * sp] and of the target at yt[t * st] (element strides sp, st >= 1):
 *   frames    F = 1 + T / 256 frames of 1024 samples, hop 256, of the signal reflect-padded by 512 samples on each side, each
 *             multiplied by the window w[1024];  S[k][f] = |sum_n frame_f[n] exp(-2 pi i k n / 1024)|, k = 0 .. 512
 *   smoothing P[i][j] = sum_{a, b < 64} h[a] h[b] S[si i + a][sj j + b],  I = (513 - 64) / si + 1,  J = (F - 64) / sj + 1
 *   loss      |P2 - P1|_F / |P1|_F / |P2|_F, P1 of the prediction and P2 of the target
 * w[1024] and h[64] are device arrays of the signals' type; tw[j] = exp(-2 pi i j / 1024), j < 1024, is the complex table of
 * fl_twiddle_fill_* for length 1024.  T must lie in [16128, 2^30] (J >= 1) and si, sj >= 1.
 *
 *   fl_avgpow_frames        F, or -1 when T is out of range
 *   fl_avgpow_work_doubles  doubles of the scratch `work` (the half-smoothed spectrogram Q[2][F][I] and the partial sums of the
 *                           combine), or -1 for bad arguments; private to the stream while the forward entry runs
 *   fl_avgpow_keep_doubles  doubles of `keep` (4 + 2 I J), or -1: what the backward entry reads again --
 *                           keep[0..3] = |P1|^2, |P2|^2, |P2 - P1|^2, loss, then P1 and P2 as doubles, [j * I + i]
 *   fl_avgpow_fwd_*         three launches: the frame kernel (both signals, one wavefront per frame: windowed reflect-indexed
 *                           load, a real transform of length 1024, magnitudes, the along-frequency half of the smoothing),
 *                           the combine (the along-frames half, P1 / P2 as (I, J) arrays of the signals' type, fixed-order
 *                           partial sums of squares in double) and the final sum, which writes keep[0..3] and loss[0]
 *   fl_avgpow_bwd_*         two launches: gframes[f][n] (F x 1024 of the signals' type, 16-byte aligned) receives the
 *                           gradient of the loss with respect to the windowed-frame samples of the prediction for the frames
 *                           f <= sj (J - 1) + 63 that the smoothing reads, and gy[t] (contiguous, T elements) =
 *                           gloss[0] times the overlap-add of those frames with the reflected margins folded back onto the
 *                           samples 1 .. 512 and T - 513 .. T - 2; samples that no used frame covers receive an exact zero.
 *                           The gradient of |X| is 0 where |X| = 0.
 * loss and gloss are device scalars of the signals' type.  Every sum is taken in a fixed order (no atomics); everything behind
 * the magnitudes is accumulated in double in both precisions. */
#ifndef FLAMO_HIP_AVGPOW_H
#define FLAMO_HIP_AVGPOW_H

#ifdef __cplusplus
extern "C" {
#endif

long fl_avgpow_frames(long T);
long fl_avgpow_work_doubles(long T, int si, int sj);
long fl_avgpow_keep_doubles(long T, int si, int sj);

int fl_avgpow_fwd_f32(const void* yp, long sp, const void* yt, long st, long T, int si, int sj, const void* w, const void* h,
                      const void* tw, void* work, void* keep, void* P1, void* P2, void* loss, void* stream);
int fl_avgpow_fwd_f64(const void* yp, long sp, const void* yt, long st, long T, int si, int sj, const void* w, const void* h,
                      const void* tw, void* work, void* keep, void* P1, void* P2, void* loss, void* stream);

int fl_avgpow_bwd_f32(const void* yp, long sp, long T, int si, int sj, const void* w, const void* h, const void* tw,
                      const void* keep, const void* gloss, void* gframes, void* gy, void* stream);
int fl_avgpow_bwd_f64(const void* yp, long sp, long T, int si, int sj, const void* w, const void* h, const void* tw,
                      const void* keep, const void* gloss, void* gframes, void* gy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLAMO_HIP_AVGPOW_H */
