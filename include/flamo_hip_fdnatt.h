/* flamo_hip_fdnatt.h -- C ABI of the delay-scaled FDN attenuation designs (csrc/fdnatt.hip), the fourth header of
 * libflamo_hip.so.
 *
 * Same conventions as flamo_hip.h (which declares the error codes and fl_last_error): every function returns FL_OK or an
 * FL_ERR_* code, pointers are device addresses, `stream` is a hipStream_t, nothing synchronises with the host and nothing
 * allocates.  One declaration per `;`, every parameter named: flamo_amd/_lib.py reads the ctypes signatures from this text.
 *
 * The attenuation filters in the feedback path of a feedback delay network take reverberation times in seconds and give
 * line n, whose delay is d[n] samples, the gain -60 d[n] / (rt fs) dB (flamo/auxiliary/reverb.py:459-552, 808-887).  These
 * entries are the step from the parameters to second-order sections b, a (3, S, N) in double -- what fl_sos_response_* and
 * fl_sos_response_bwd_* take -- and its adjoint.  `delays` holds N doubles.  A parameter vector is float32 (`*_f32` = 1) or
 * float64 (0); its gradient is written in the same type.
 *
 *   fl_fdn_geq_sections        rt (nb) -> the graphic equaliser's nb sections per line: g = 10^((-60 / (rt[k] fs)) d[n] / 20),
 *                              then the design of fl_geq_sections (same band constants `consts`, same float32 roundings)
 *   fl_fdn_geq_sections_bwd    gb / ga: dL/db and dL/da as nblk blocks of (3, nb, N) doubles, blk_stride elements apart (the
 *                              block partials of fl_sos_response_bwd_*), summed in block order -> grt (nb).  One wavefront per
 *                              band: lanes stride over the lines, then a fixed butterfly; no atomics
 *   fl_fdn_shelf1_sections     p = (rt at DC, crossover w_c in radians) -> one first-order shelving section per line, third
 *                              taps zero: t = tan(clamp(w_c, 0, pi) / 2), k = 10^(slope_dc d / 20) / gN, gN = 10^(slope_nyq d / 20),
 *                              slope_dc = -60 / (rt fs);  b = (f32(t sqrt(k) + 1) gN, f32(t sqrt(k) - 1) gN, 0),
 *                              a = (f32(t / sqrt(k) + 1), f32(t / sqrt(k) - 1), 0), f32 = rounded to float32
 *   fl_fdn_shelf1_sections_bwd the same block partials with nb = 1 -> gp (2); the clamp passes the gradient on [0, pi].  One
 *                              wavefront, the same fixed order */
#ifndef FLAMO_HIP_FDNATT_H
#define FLAMO_HIP_FDNATT_H

#ifdef __cplusplus
extern "C" {
#endif

int fl_fdn_geq_sections(const void* rt, int rt_f32, const void* delays, int nb, int N, double fs, const void* consts, void* b,
                        void* a, void* stream);
int fl_fdn_geq_sections_bwd(const void* rt, int rt_f32, const void* delays, const void* gb, const void* ga, long blk_stride,
                            int nblk, int nb, int N, double fs, const void* consts, void* grt, void* stream);

int fl_fdn_shelf1_sections(const void* p, int p_f32, const void* delays, int N, double fs, double slope_nyq, void* b, void* a,
                           void* stream);
int fl_fdn_shelf1_sections_bwd(const void* p, int p_f32, const void* delays, const void* gb, const void* ga, long blk_stride,
                               int nblk, int N, double fs, double slope_nyq, void* gp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLAMO_HIP_FDNATT_H */
