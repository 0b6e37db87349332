/* flamo_hip_filterbank.h -- C ABI of the frequency-domain band split (csrc/filterbank.hip), the eighth header of
 * libflamo_hip.so.
 *
 * Same conventions as flamo_hip.h (which declares the error codes and fl_last_error): every fl_*_f32 / _f64 function returns
 * FL_OK or an FL_ERR_* code, pointers are device addresses, `stream` is a hipStream_t, nothing synchronises with the host and
 * nothing allocates.  One declaration per `;`, every parameter named: flamo_amd/_lib.py reads the ctypes signatures from this
 * text.
 *
 * The split multiplies the M bins of `rows` spectra by the responses of K bands, sampled on the grid w_k = pi k / M,
 * k = 0 .. M - 1 (M samples of [0, pi): the grid of a `freqz` with M points, NOT 2 pi k / nfft):
 *   forward    Y[r, j, k] = H_j(w_k) X[r, k]
 *   backward   gX[r, k]   = sum_j conj(H_j(w_k)) gY[r, j, k]
 * X and gX are rows of M complex elements `pitch_x` elements apart (what the real transform writes: signal-planar, bins
 * contiguous); Y and gY are rows of M complex elements `pitch_y` apart, row r K + j the band j of spectrum r (what the inverse
 * real transform reads).  Complex elements have the entry's precision (_f32: two floats, _f64: two doubles).  Only the M
 * elements of a row are read or written, never its padding.
 *
 * A band is given by its zeros, poles and gain, H(z) = g prod (z - z_i) / prod (z - p_i), handed over about z = 1: `consts`
 * holds FL_FILTERBANK_BAND doubles per band (in both precisions) -- the number of zeros, the number of poles, g, one unused --
 * then FL_FILTERBANK_MAXP pairs (re, im) of 1 - z_i and FL_FILTERBANK_MAXP pairs of 1 - p_i, formed in float64 by the caller.
 * The kernels evaluate
 *   u = z - 1 = -2 sin^2(w / 2) + i sin w,      H = g prod (u + (1 - z_i)) / prod (u + (1 - p_i))
 * in DOUBLE in both precisions, once per (bin, band) forward (reused over the rows) and once per (bin, band, four rows)
 * backward, and never write a response to memory.  Why this form and why double: the poles of a low band lie 1e-3 and less
 * from z = 1, where b0 + b1 z^-1 + b2 z^-2 in float32 loses the response altogether (3.6e-2 of a peak of 1) and the plain
 * factors z - p_i in float32 still 2.4e-4; about z = 1 the small differences are formed exactly, and in double the products of
 * up to 16 factors of 1e-3 (1e-48) stay far inside the exponent range, so one complex division per response is all that is
 * needed.  The arithmetic is a few hundred FMAs per response beside 8 to 16 bytes stored per row: the kernels are bound by
 * their stores (by the launch at the sizes of one impulse response).  The kernels clamp the two counts to FL_FILTERBANK_MAXP.
 *
 *   fl_filterbank_supports     1 when the kernels take K bands with at most `max_roots` zeros or poles each
 *                              (1 <= K <= FL_FILTERBANK_MAXK, 0 <= max_roots <= FL_FILTERBANK_MAXP), else 0
 *   fl_filterbank_const_elems  doubles of `consts` for K bands, or -1
 *   fl_filterbank_fwd_*        ONE launch: a thread per (bin, band), a loop over the rows
 *   fl_filterbank_bwd_*        ONE launch: a thread per (bin, four rows), the band sum in registers, a fixed order
 * Sizes: rows >= 1, 1 <= M <= 2^30, pitch_x, pitch_y >= M, rows K < 2^31. */
#ifndef FLAMO_HIP_FILTERBANK_H
#define FLAMO_HIP_FILTERBANK_H

#define FL_FILTERBANK_MAXK 34
#define FL_FILTERBANK_MAXP 16
#define FL_FILTERBANK_BAND 68

#ifdef __cplusplus
extern "C" {
#endif

int fl_filterbank_supports(int K, int max_roots);
long fl_filterbank_const_elems(int K);

int fl_filterbank_fwd_f32(const void* X, long pitch_x, long rows, long M, const void* consts, int K, void* Y, long pitch_y,
                          void* stream);
int fl_filterbank_fwd_f64(const void* X, long pitch_x, long rows, long M, const void* consts, int K, void* Y, long pitch_y,
                          void* stream);

int fl_filterbank_bwd_f32(const void* gY, long pitch_y, long rows, long M, const void* consts, int K, void* gX, long pitch_x,
                          void* stream);
int fl_filterbank_bwd_f64(const void* gY, long pitch_y, long rows, long M, const void* consts, int K, void* gX, long pitch_x,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLAMO_HIP_FILTERBANK_H */
