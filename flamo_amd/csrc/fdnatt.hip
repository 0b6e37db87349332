// Delay-scaled attenuation filters of a feedback delay network (flamo/auxiliary/reverb.py:459-552 parallelFDNGEQ,
// 808-887 parallelFirstOrderShelving): the step from the parameters -- reverberation times in seconds -- to the second-order
// sections the cascade kernels of response.hip evaluate, and its adjoint.  Line n with a delay of d[n] samples is attenuated
// by -60 d[n] / (rt fs) dB per pass, so that every line decays by 60 dB in rt seconds.
//
// The reference loops over the delay lines in Python and designs one equaliser per line (about 150 elementwise launches per
// line, each way); here one thread designs one (band, line) section and one wavefront per parameter sums the adjoint over the
// lines.  The section arithmetic is geq_section_vals / geq_design_bwd of response_common.h, the design of fl_geq_sections,
// but for the scalings of the two shelves (shelf_section_vals below): every coefficient is rounded to float32 exactly where the
// reference's float32 buffers round it.
//
// Every sum is taken in a fixed order: a lane adds its lines (n = lane, lane + 64, ...) in ascending order, each from block
// partials added in block order, then the 64 lanes combine in a butterfly of fixed shape.  No atomics: two runs give the same
// bits.
#include "response_common.h"
#include "../../include/flamo_hip_fdnatt.h"

namespace fl {
namespace fdnatt {

constexpr double LN10_OVER_20 = 2.302585092994045684 / 20.0;

__device__ inline double load_param(const void* p, int f32, int i) {
    return f32 ? (double)reinterpret_cast<const float*>(p)[i] : reinterpret_cast<const double*>(p)[i];
}
__device__ inline void store_param(void* p, int f32, int i, double v) {
    if (f32) reinterpret_cast<float*>(p)[i] = (float)v;
    else reinterpret_cast<double*>(p)[i] = v;
}
// linear gain of a line of d samples under the slope s dB per sample: the reference forms s * d, then 10^(./20)
__device__ inline double line_gain(double slope, double d) { return pow(10.0, slope * d / 20.0); }

// dL/d(b, a) of section idx (of st per tap) from nblk blocks blk_stride elements apart, added in block order
__device__ inline void sum_blocks(const double* __restrict__ gb, const double* __restrict__ ga, long blk_stride, int nblk, int idx,
                                  int st, double* B, double* A) {
    B[0] = B[1] = B[2] = A[0] = A[1] = A[2] = 0.0;
    for (int blk = 0; blk < nblk; ++blk) {
        const double* pb = gb + (size_t)blk * blk_stride + idx;
        const double* pa = ga + (size_t)blk * blk_stride + idx;
        B[0] += pb[0]; B[1] += pb[st]; B[2] += pb[2 * (size_t)st];
        A[0] += pa[0]; A[1] += pa[st]; A[2] += pa[2 * (size_t)st];
    }
}

// ---------------------------------------------------------------- graphic equaliser: rt (nb) -> b, a (3, nb, N)
// The two shelving sections of THIS class.  reverb.py:523-524 hands eq.geq one-element gain VECTORS where dsp.GEQ hands it
// scalars, and torch's type promotion then keeps the whole-vector scalings g^(1/2) b and a g (functional.py:615-619) in
// float64: their products are rounded to float32 once, when stored, where geq_section_vals -- the scalar choreography --
// multiplies two float32 values.  The difference is a float32 ulp per tap, which the cancellation b0 + b1 + b2 of a shelf
// near DC turns into 2e-3 of the response, so the rounding points here are the reference's.  The flat gain and the peaking
// bands round alike in both and come from geq_section_vals; the adjoint (geq_design_bwd) does not see roundings.
__device__ inline void shelf_section_vals(double g, bool high, double t2, double stq, double* bb, double* aa) {
    const double u = sqrt(g), q = sqrt(u);
    const double p0 = f32r(u * t2 + stq * q + 1), p1 = f32r(2 * u * t2 - 2), p2 = f32r(u * t2 - stq * q + 1);
    const double d0 = f32r(u + stq * q + t2), d1 = f32r(2 * t2 - 2 * u), d2 = f32r(u - stq * q + t2);
    const double s0 = f32r(u * p0), s1 = f32r(u * p1), s2 = f32r(u * p2);
    if (!high) {
        bb[0] = s0; bb[1] = s1; bb[2] = s2; aa[0] = d0; aa[1] = d1; aa[2] = d2;
    } else {
        bb[0] = f32r(d0 * g); bb[1] = f32r(d1 * g); bb[2] = f32r(d2 * g); aa[0] = s0; aa[1] = s1; aa[2] = s2;
    }
}

__global__ void __launch_bounds__(256) geq_kernel(const void* __restrict__ rt, int rt_f32, const double* __restrict__ delays, int nb,
                                                  int N, double fs, const double* __restrict__ k, double* __restrict__ b,
                                                  double* __restrict__ a) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int st = nb * N;
    if (idx >= st) return;
    const int band = idx / N, n = idx - band * N;
    const double g = line_gain(-60.0 / (load_param(rt, rt_f32, band) * fs), delays[n]);
    int ia, ib;
    geq_band_const_idx(band, nb, &ia, &ib);
    double bb[3], aa[3];
    if (band == 1 || band == nb - 1) shelf_section_vals(g, band != 1, k[ia], k[ib], bb, aa);
    else geq_section_vals(g, band, nb, k[ia], k[ib], bb, aa);
    b[idx] = bb[0]; b[idx + st] = bb[1]; b[idx + 2 * (size_t)st] = bb[2];
    a[idx] = aa[0]; a[idx + st] = aa[1]; a[idx + 2 * (size_t)st] = aa[2];
}

// one wavefront per band
__global__ void __launch_bounds__(64) geq_bwd_kernel(const void* __restrict__ rt, int rt_f32, const double* __restrict__ delays,
                                                     const double* __restrict__ gb, const double* __restrict__ ga, long blk_stride,
                                                     int nblk, int nb, int N, double fs, const double* __restrict__ k,
                                                     void* __restrict__ grt) {
    const int band = blockIdx.x, lane = threadIdx.x;
    if (band >= nb) return;
    const double r = load_param(rt, rt_f32, band);
    const double slope = -60.0 / (r * fs);
    double v = 0.0;
    for (int n = lane; n < N; n += 64) {
        const double d = delays[n];
        const double g = line_gain(slope, d);
        double B[3], A[3];
        sum_blocks(gb, ga, blk_stride, nblk, band * N + n, nb * N, B, A);
        const double dg = geq_design_bwd(band, nb, g, k, B[0], B[1], B[2], A[0], A[1], A[2]);
        v += dg * g * LN10_OVER_20 * 60.0 * d / (r * r * fs);      // dg/drt
    }
    v = wave_sum(v);
    if (lane == 0) store_param(grt, rt_f32, band, v);
}

// ---------------------------------------------------------------- first-order shelving: (rt at DC, w_c) -> b, a (3, 1, N)
struct Shelf {
    double t, sk, gN;      // tan(w_c / 2), sqrt(k), the line's gain at the Nyquist frequency
};
__device__ inline Shelf shelf_of(double rt_dc, double wc, double d, double fs, double slope_nyq) {
    Shelf s;
    const double w = fmin(fmax(wc, 0.0), 3.14159265358979323846);
    s.t = tan(w / 2);
    s.gN = line_gain(slope_nyq, d);
    s.sk = sqrt(line_gain(-60.0 / (rt_dc * fs), d) / s.gN);
    return s;
}

__global__ void __launch_bounds__(256) shelf1_kernel(const void* __restrict__ p, int p_f32, const double* __restrict__ delays, int N,
                                                     double fs, double slope_nyq, double* __restrict__ b, double* __restrict__ a) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const Shelf s = shelf_of(load_param(p, p_f32, 0), load_param(p, p_f32, 1), delays[n], fs, slope_nyq);
    b[n] = f32r(s.t * s.sk + 1) * s.gN; b[n + N] = f32r(s.t * s.sk - 1) * s.gN; b[n + 2 * (size_t)N] = 0.0;
    a[n] = f32r(s.t / s.sk + 1);        a[n + N] = f32r(s.t / s.sk - 1);        a[n + 2 * (size_t)N] = 0.0;
}

// one wavefront
__global__ void __launch_bounds__(64) shelf1_bwd_kernel(const void* __restrict__ p, int p_f32, const double* __restrict__ delays,
                                                        const double* __restrict__ gb, const double* __restrict__ ga,
                                                        long blk_stride, int nblk, int N, double fs, double slope_nyq,
                                                        void* __restrict__ gp) {
    const int lane = threadIdx.x;
    const double r = load_param(p, p_f32, 0), wc = load_param(p, p_f32, 1);
    double v_rt = 0.0, v_t = 0.0;
    for (int n = lane; n < N; n += 64) {
        const double d = delays[n];
        const Shelf s = shelf_of(r, wc, d, fs, slope_nyq);
        double B[3], A[3];
        sum_blocks(gb, ga, blk_stride, nblk, n, N, B, A);
        const double Bs = (B[0] + B[1]) * s.gN, As = A[0] + A[1];
        // the taps depend on t sqrt(k) (numerator) and t / sqrt(k) (denominator)
        const double d_sk = Bs * s.t - As * s.t / (s.sk * s.sk);
        v_t += Bs * s.sk + As / s.sk;
        // sqrt(k) = 10^((slope_dc - slope_nyq) d / 40): d sqrt(k) / d rt = sqrt(k) (ln 10 / 40) 60 d / (rt^2 fs)
        v_rt += d_sk * s.sk * (0.5 * LN10_OVER_20) * 60.0 * d / (r * r * fs);
    }
    v_rt = wave_sum(v_rt);
    v_t = wave_sum(v_t);
    if (lane == 0) {
        const bool inside = wc >= 0.0 && wc <= 3.14159265358979323846;      // torch.clamp passes the gradient on the closed range
        const double t = tan(fmin(fmax(wc, 0.0), 3.14159265358979323846) / 2);
        store_param(gp, p_f32, 0, v_rt);
        store_param(gp, p_f32, 1, inside ? v_t * 0.5 * (1.0 + t * t) : 0.0);
    }
}

}  // namespace fdnatt
}  // namespace fl

using namespace fl;
using namespace fl::fdnatt;

extern "C" int fl_fdn_geq_sections(const void* rt, int rt_f32, const void* delays, int nb, int N, double fs, const void* consts,
                                   void* b, void* a, void* stream) {
    FL_REQUIRE(rt && delays && consts && b && a, "fdn_geq_sections: null pointer");
    FL_REQUIRE(nb >= 4 && N > 0 && (long)nb * N < (1L << 30) && fs > 0, "fdn_geq_sections: need >= 4 bands (gain, two shelves, one peak), N > 0, fs > 0");
    hipLaunchKernelGGL(geq_kernel, dim3(cdiv_i((long)nb * N, 256)), dim3(256), 0, (hipStream_t)stream, rt, rt_f32, (const double*)delays,
                       nb, N, fs, (const double*)consts, (double*)b, (double*)a);
    FL_CHECK_LAUNCH("fdn_geq_sections");
    return FL_OK;
}

extern "C" int fl_fdn_geq_sections_bwd(const void* rt, int rt_f32, const void* delays, const void* gb, const void* ga,
                                       long blk_stride, int nblk, int nb, int N, double fs, const void* consts, void* grt,
                                       void* stream) {
    FL_REQUIRE(rt && delays && gb && ga && consts && grt, "fdn_geq_sections_bwd: null pointer");
    FL_REQUIRE(nb >= 4 && N > 0 && (long)nb * N < (1L << 30) && fs > 0 && nblk >= 1 && blk_stride >= 0, "fdn_geq_sections_bwd: bad sizes");
    hipLaunchKernelGGL(geq_bwd_kernel, dim3(nb), dim3(64), 0, (hipStream_t)stream, rt, rt_f32, (const double*)delays, (const double*)gb,
                       (const double*)ga, blk_stride, nblk, nb, N, fs, (const double*)consts, grt);
    FL_CHECK_LAUNCH("fdn_geq_sections_bwd");
    return FL_OK;
}

extern "C" int fl_fdn_shelf1_sections(const void* p, int p_f32, const void* delays, int N, double fs, double slope_nyq, void* b,
                                      void* a, void* stream) {
    FL_REQUIRE(p && delays && b && a, "fdn_shelf1_sections: null pointer");
    FL_REQUIRE(N > 0 && N < (1 << 30) && fs > 0, "fdn_shelf1_sections: need N > 0, fs > 0");
    hipLaunchKernelGGL(shelf1_kernel, dim3(cdiv_i(N, 256)), dim3(256), 0, (hipStream_t)stream, p, p_f32, (const double*)delays, N, fs,
                       slope_nyq, (double*)b, (double*)a);
    FL_CHECK_LAUNCH("fdn_shelf1_sections");
    return FL_OK;
}

extern "C" int fl_fdn_shelf1_sections_bwd(const void* p, int p_f32, const void* delays, const void* gb, const void* ga,
                                          long blk_stride, int nblk, int N, double fs, double slope_nyq, void* gp, void* stream) {
    FL_REQUIRE(p && delays && gb && ga && gp, "fdn_shelf1_sections_bwd: null pointer");
    FL_REQUIRE(N > 0 && N < (1 << 30) && fs > 0 && nblk >= 1 && blk_stride >= 0, "fdn_shelf1_sections_bwd: bad sizes");
    hipLaunchKernelGGL(shelf1_bwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p, p_f32, (const double*)delays, (const double*)gb,
                       (const double*)ga, blk_stride, nblk, N, fs, slope_nyq, gp);
    FL_CHECK_LAUNCH("fdn_shelf1_sections_bwd");
    return FL_OK;
}
