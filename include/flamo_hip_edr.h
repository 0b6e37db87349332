/* flamo_hip_edr.h -- C ABI of the mel energy-decay-relief criterion (csrc/edr.hip), the sixth header of libflamo_hip.so.
 *
 * Same conventions as flamo_hip.h (which declares the error codes and fl_last_error): every fl_*_f32 / _f64 function returns
 * FL_OK or an FL_ERR_* code, pointers are device addresses, `stream` is a hipStream_t, nothing synchronises with the host and
 * nothing allocates.  One declaration per `;`, every parameter named: flamo_amd/_lib.py reads the ctypes signatures from this
 * text.
 *
 * The criterion compares a prediction and a target of shape (B, T, N); element (b, t, c) of the prediction is at
 * yp[b * spb + t * spt + c * spc] and of the target at yt[b * stb + t * stt + c * stc] (element strides of any sign, nothing
 * is copied).  Every (b, c) column is one row, B N rows.
 *   frames   F = 1 + T / hop frames of n_fft samples of the row reflect-padded by n_fft / 2 on each side, each multiplied by
 *            the window of win samples centred in the frame (left pad (n_fft - win) / 2);  X[k] its transform, k = 0 .. n_fft/2
 *   P        re^2 + im^2 (its gradient at an exact zero is 0)
 *   m        W P, W the (64, n_fft / 2 + 1) mel basis: 64 band energies per frame
 *   E        E[f] = sum_{f' >= f} m[f']^2, the backward integral over the frames of a row and band
 *   edr      10 log10 E[f], or with energy_norm 10 log10 (E[f] / E[0])
 *   clip     where the TARGET's E_t[f] == 0 exactly both entries become eps: 0 to the numerator, eps to the denominator, and
 *            no gradient
 *   loss     sum |edr_t - edr_p| / sum |edr_t| over all rows, bands and frames at once (inf where E_p[f] == 0 < E_t[f])
 * Sizes the kernels take: n_fft a power of two from 256 to 2048, 1 <= win <= n_fft, hop >= 1, n_fft / 2 < T <= 2^30,
 * B, N >= 1, fewer than 2^31 frames and at most 2^38 samples in all.
 * wtab holds the window (win DOUBLES, in float32 too); tw[j] = exp(-2 pi i j / 2048), j < 2048, is the complex DOUBLE table
 * of fl_twiddle_fill_f64 for length 2048: both precisions transform in double, and only the signals, gframes, gy, loss and
 * gloss have the signals' type.
 * The mel basis is the caller's host matrix, handed over as two tables.  melidx (fl_edr_mel_ints int32): start[64], count[64],
 * offset[64] -- band j holds the bins start[j] .. start[j] + count[j] - 1, their weights at melw[offset[j] ..] -- then
 * band[n_fft / 2 + 1]: bin k lies in the bands band[k] and band[k] + 1 and no other (0 <= band[k] <= 62).  melw
 * (fl_edr_mel_doubles doubles): the nnz packed weights, then for every bin k its weights in band[k] and in band[k] + 1.
 * The kernels clamp what they read from melidx to the arrays it indexes.
 *
 *   fl_edr_frames        F, or -1 for sizes the kernels do not take (the support query)
 *   fl_edr_band_doubles  B N F 64: the doubles of `kept` and of `gmel`, and half those of `mel` (prediction, then target,
 *                        each [row][frame][64]), or -1
 *   fl_edr_gframe_elems  elements of `gframes` (B N F win), or -1
 *   fl_edr_keep_doubles  doubles of `keep` (1): 1 / D, D = sum |edr_t|, which the backward entry reads again
 *   fl_edr_fwd_*         THREE launches: the frame kernel (one wavefront per (row, frame): windowed reflect-indexed loads of
 *                        prediction and target, two real transforms, |X|^2 in LDS, lane j sums band j: 64 doubles per frame
 *                        and signal into `mel`), the relief kernel (one workgroup per row, lane = band: the backward integral
 *                        over frames in two walks of 16 segments, the dB values, the clip, the row's two sums into
 *                        rowsum[2 B N]; with `kept` not null also sign(edr_t - edr_p) (10 / ln 10) / E_p[f] per entry, 0
 *                        where clipped, frame 0 with the energy_norm term folded in) and the final kernel, which writes keep
 *                        and loss[0].  kept may be null when no gradient is wanted.
 *   fl_edr_bwd_*         THREE launches: the prefix kernel (gmel[f'] = -2 m_p[f'] / D times the sum of kept[f], f <= f'), the
 *                        frame kernel (the prediction's transform recomputed, dL/dP gathered from the two bands of a bin,
 *                        dL/dX = 2 X dL/dP, the adjoint of the real-transform split, the inverse transform; the win samples
 *                        under the window go to gframes) and the overlap-add, a gather per sample in a fixed order with the
 *                        reflected margins folded back: gy (contiguous (B, T, N)) = gloss[0] times the gradient of the loss.
 * loss and gloss are device scalars of the signals' type; mel, kept, rowsum, keep and gmel device doubles.  Every sum is taken
 * in a fixed order (no atomics); everything behind the loads of the signals is a double in both precisions. */
#ifndef FLAMO_HIP_EDR_H
#define FLAMO_HIP_EDR_H

#ifdef __cplusplus
extern "C" {
#endif

long fl_edr_frames(long B, long T, long N, int nfft, int hop, int win);
long fl_edr_band_doubles(long B, long T, long N, int nfft, int hop, int win);
long fl_edr_gframe_elems(long B, long T, long N, int nfft, int hop, int win);
long fl_edr_keep_doubles(void);
long fl_edr_mel_ints(int nfft);
long fl_edr_mel_doubles(int nfft, int nnz);

int fl_edr_fwd_f32(const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long T,
                   long N, int nfft, int hop, int win, const void* wtab, const void* tw, const void* melidx, const void* melw,
                   int nnz, int energy_norm, double eps, void* mel, void* kept, void* rowsum, void* keep, void* loss,
                   void* stream);
int fl_edr_fwd_f64(const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long T,
                   long N, int nfft, int hop, int win, const void* wtab, const void* tw, const void* melidx, const void* melw,
                   int nnz, int energy_norm, double eps, void* mel, void* kept, void* rowsum, void* keep, void* loss,
                   void* stream);

int fl_edr_bwd_f32(const void* yp, long spb, long spt, long spc, long B, long T, long N, int nfft, int hop, int win,
                   const void* wtab, const void* tw, const void* melidx, const void* melw, int nnz, const void* mel,
                   const void* kept, const void* keep, const void* gloss, void* gmel, void* gframes, void* gy, void* stream);
int fl_edr_bwd_f64(const void* yp, long spb, long spt, long spc, long B, long T, long N, int nfft, int hop, int win,
                   const void* wtab, const void* tw, const void* melidx, const void* melw, int nnz, const void* mel,
                   const void* kept, const void* keep, const void* gloss, void* gmel, void* gframes, void* gy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLAMO_HIP_EDR_H */
