/* flamo_hip_edc.h -- C ABI of the energy-decay-curve criterion (csrc/edc.hip), the second header of libflamo_hip.so.
 *
 * Same conventions as flamo_hip.h (which declares the error codes, fl_last_error and fl_mean_square_scratch_bytes): every
 * function returns FL_OK or an FL_ERR_* code, pointers are device addresses, `stream` is a hipStream_t, nothing synchronises
 * with the host and nothing allocates.  One declaration per `;`, every parameter named: flamo_amd/_lib.py reads the ctypes
 * signatures from this text.
 *
 * The signal y holds B items of T samples in N channels; only the first Tk samples are kept (the reference drops the last
 * 0.5 %: flamo/optimize/loss.py:742-747).  Two memory layouts, chosen by `planar`:
 *   planar = 0   y[b][t][c] at (b*T + t)*N + c                 contiguous (B, T, N), `pitch` is ignored
 *   planar = 1   y[b][t][c] at (b*N + c)*pitch + t             signal-planar rows, pitch >= T, padding neither read nor written
 * Time is cut into tiles of fl_edc_tile() samples, nt = ceil(Tk / tile) of them per column; a "tile array" holds
 * B*N*nt doubles, [(b*N + c)*nt + j].  E[b][s][c] = sum_{s <= t < Tk} y[b][t][c]^2 (Schroeder's backward integral),
 * e = 10 log10(E / Z), Z = E[b][0][c] with energy_norm and 1 without.
 *
 *   fl_edc_tile_sums_*   tsum[(b*N + c)*nt + j] = sum of y^2 over tile j
 *   fl_edc_curve_*       edb[b][s][c] = e, contiguous (B, Tk, N), never clipped.  den (optional, null = absent) receives
 *                        mean(e~^2) over B*Tk*N entries, e~ = e with the entries below max_s e - 60 set to -180 when `clip`
 *                        (needs `scratch`: fl_mean_square_scratch_bytes() bytes private to the stream)
 *   fl_edc_loss_*        loss[0] = mean(m (e - e*)^2) [/ den[0] when den is given], e of the prediction y, e* = edb_true
 *                        (a curve of fl_edc_curve_*, with tsum_true the tile sums it was made from), m = 0 where
 *                        `clip` and e* < e*[b][0][c] - 60, else 1.  w (optional, null = no gradient wanted) receives
 *                        m (e - e*) / E in y's own layout, wsum / wesum the tile sums of w and of m (e - e*)
 *   fl_edc_bwd_*         gy[b][t][c] = 2 y k (sum_{s <= t} w[s] - (energy_norm ? sum_s wesum / E[b][0][c] : 0)) for t < Tk and
 *                        0 for Tk <= t < T, k = gloss[0] * (2 / (B Tk N)) * (10 / ln 10) [/ den[0] when den is given];
 *                        gy in y's layout
 * loss, gloss, den are device scalars of y's type.  Every sum is taken in a fixed order (no atomics); tile sums, carries
 * and loss partials are doubles in both precisions. */
#ifndef FLAMO_HIP_EDC_H
#define FLAMO_HIP_EDC_H

#ifdef __cplusplus
extern "C" {
#endif

/* samples per time tile (one wavefront's share of a column) */
int fl_edc_tile(void);

int fl_edc_tile_sums_f32(const void* y, int planar, int B, long T, long Tk, int N, long pitch, void* tsum, void* stream);
int fl_edc_tile_sums_f64(const void* y, int planar, int B, long T, long Tk, int N, long pitch, void* tsum, void* stream);

int fl_edc_curve_f32(const void* y, int planar, int B, long T, long Tk, int N, long pitch, const void* tsum, int energy_norm,
                     int clip, void* edb, void* den, void* scratch, void* stream);
int fl_edc_curve_f64(const void* y, int planar, int B, long T, long Tk, int N, long pitch, const void* tsum, int energy_norm,
                     int clip, void* edb, void* den, void* scratch, void* stream);

int fl_edc_loss_f32(const void* y, int planar, int B, long T, long Tk, int N, long pitch, const void* tsum, const void* edb_true,
                    const void* tsum_true, int energy_norm, int clip, const void* den, void* w, void* wsum, void* wesum,
                    void* loss, void* scratch, void* stream);
int fl_edc_loss_f64(const void* y, int planar, int B, long T, long Tk, int N, long pitch, const void* tsum, const void* edb_true,
                    const void* tsum_true, int energy_norm, int clip, const void* den, void* w, void* wsum, void* wesum,
                    void* loss, void* scratch, void* stream);

int fl_edc_bwd_f32(const void* y, int planar, int B, long T, long Tk, int N, long pitch, const void* tsum, const void* w,
                   const void* wsum, const void* wesum, const void* gloss, const void* den, int energy_norm, void* gy,
                   void* stream);
int fl_edc_bwd_f64(const void* y, int planar, int B, long T, long Tk, int N, long pitch, const void* tsum, const void* w,
                   const void* wsum, const void* wesum, const void* gloss, const void* den, int energy_norm, void* gy,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLAMO_HIP_EDC_H */
