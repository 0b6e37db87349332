// Average-power criterion (gfx950 / MI355X): the reference's AveragePower (flamo/optimize/loss.py:462-549), whose torch form is
// two torch.stft, two abs, two conv2d with a 64 x 64 kernel, three norms and two divisions, and the backward of all of it.
//
//   S[k][f] = |X[k][f]|,  X[.][f] = the length-1024 transform of the windowed frame f of the reflect-padded signal (hop 256)
//   P[i][j] = sum_{a, b < 64} h[a] h[b] S[si i + a][sj j + b]          loss = |P2 - P1|_F / |P1|_F / |P2|_F
//
// The framed transform is one wavefront per frame, the n_fft = 1024, hop = 256, full-window instance of framed.h in the
// signal's precision: 512 complex values, 8 per lane, split into the 513 bins of the real transform.  The
// spectrogram never reaches memory: the frame's magnitudes stay in LDS and are smoothed along frequency there, so that a frame
// leaves I doubles (Q[f][i]); the combine smooths along the frames.  The backward pass rebuilds dL/dQ and dL/dS of a frame from
// the kept P1, P2 and the three sums of squares, recomputes the frame's transform (cheaper than keeping 513 x F complex values),
// runs the adjoint of the split and the inverse transform, and an overlap-add gathers the frames' gradients per sample.
// Every sum has a fixed order; everything behind the magnitudes is a double in both precisions.
#include "framed.h"
#include "../../include/flamo_hip_avgpow.h"

namespace fl {
namespace avgpow {

constexpr int NFFT = 1024, HOP = 256, NB = NFFT / 2 + 1, HALF = NFFT / 2, WIN = 64;
constexpr long T_MIN = (long)HOP * (WIN - 1), T_MAX = 1L << 30;      // J >= 1 needs F = 1 + T / 256 >= 64
constexpr int PL = HALF / 64, ZLDS = HALF + 64;                      // framed.h: complex values per lane, its LDS array
constexpr framed::Frame FRAME{HOP, NFFT, 0};                         // the window covers the whole frame
constexpr int IMAX = NB - WIN + 1;                                   // rows of P at si = 1

struct Plan {
    long T, F;
    int si, sj, I, J;
    long nb;       // workgroups of the combine
    long last;     // last frame the smoothing reads
};
static bool make_plan(long T, int si, int sj, Plan& p) {
    if (T < T_MIN || T > T_MAX || si < 1 || sj < 1) return false;
    p.T = T; p.si = si; p.sj = sj;
    p.F = 1 + T / HOP;
    p.I = (NB - WIN) / si + 1;
    p.J = (int)((p.F - WIN) / sj + 1);
    p.nb = ((long)p.I * p.J + 255) / 256;
    p.last = (long)sj * (p.J - 1) + WIN - 1;
    return true;
}

// ---------------------------------------------------------------- forward: a frame's magnitudes, smoothed along frequency
template <typename T>
__global__ void __launch_bounds__(64) avgpow_frames_kernel(const T* __restrict__ yp, long sp, const T* __restrict__ yt, long st,
                                                           Plan p, const T* __restrict__ w, const T* __restrict__ h,
                                                           const cx<T>* __restrict__ tw, double* __restrict__ Q) {
    __shared__ cx<T> A[ZLDS];
    __shared__ T S[NB + 7];
    __shared__ double hd[WIN];
    const int lane = threadIdx.x;
    const int sig = blockIdx.x >= p.F ? 1 : 0;
    const long f = blockIdx.x - (sig ? p.F : 0);
    hd[lane] = (double)h[lane];
    [[clang::always_inline]] framed::frame_transform<T, T, PL, NFFT>(sig ? yt : yp, sig ? st : sp, p.T, f, FRAME, w, tw, A, lane);
    for (int k = lane; k < NB; k += 64) {
        const cx<T> x = framed::split_bin<T, PL, NFFT>(A, tw, k);
        S[k] = hypot(x.x, x.y);
    }
    __syncthreads();
    double* q = Q + ((long)sig * p.F + f) * p.I;
    for (int i = lane; i < p.I; i += 64) {
        double acc = 0.0;
#pragma unroll 8
        for (int a = 0; a < WIN; ++a) acc += hd[a] * (double)S[p.si * i + a];
        q[i] = acc;
    }
}

// ---------------------------------------------------------------- combine: smoothing along the frames, partial sums of squares
template <typename T>
__global__ void __launch_bounds__(256) avgpow_combine_kernel(const double* __restrict__ Q, Plan p, const T* __restrict__ h,
                                                            double* __restrict__ keep, T* __restrict__ P1, T* __restrict__ P2,
                                                            double* __restrict__ partial) {
    __shared__ double hd[WIN];
    __shared__ double red[3][4];
    if (threadIdx.x < WIN) hd[threadIdx.x] = (double)h[threadIdx.x];
    __syncthreads();
    const long n = (long)p.I * p.J, e = (long)blockIdx.x * 256 + threadIdx.x;
    double s1 = 0.0, s2 = 0.0, sd = 0.0;
    if (e < n) {
        const int i = (int)(e % p.I), j = (int)(e / p.I);
        const double* q1 = Q + ((long)p.sj * j) * p.I + i;
        const double* q2 = q1 + p.F * p.I;
        double a1 = 0.0, a2 = 0.0;
#pragma unroll 8
        for (int b = 0; b < WIN; ++b) {
            a1 += hd[b] * q1[(long)b * p.I];
            a2 += hd[b] * q2[(long)b * p.I];
        }
        keep[4 + e] = a1;
        keep[4 + n + e] = a2;
        P1[(long)i * p.J + j] = (T)a1;
        P2[(long)i * p.J + j] = (T)a2;
        s1 = a1 * a1;
        s2 = a2 * a2;
        sd = (a2 - a1) * (a2 - a1);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    sd = wave_sum(sd);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wave] = s1;
        red[1][wave] = s2;
        red[2][wave] = sd;
    }
    __syncthreads();
    if (threadIdx.x < 3) partial[threadIdx.x * p.nb + blockIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// one wavefront: the three sums in a fixed order, the loss
template <typename T>
__global__ void __launch_bounds__(64) avgpow_final_kernel(const double* __restrict__ partial, long nb, double* __restrict__ keep,
                                                         T* __restrict__ loss) {
    double s[3];
    for (int c = 0; c < 3; ++c) {
        double a = 0.0;
        for (long b = threadIdx.x; b < nb; b += 64) a += partial[c * nb + b];
        s[c] = wave_sum(a);
    }
    if (threadIdx.x == 0) {
        const double l = sqrt(s[2]) / sqrt(s[0]) / sqrt(s[1]);
        keep[0] = s[0];
        keep[1] = s[1];
        keep[2] = s[2];
        keep[3] = l;
        loss[0] = (T)l;
    }
}

// ---------------------------------------------------------------- backward: the gradient of a frame's windowed samples
template <typename T>
__global__ void __launch_bounds__(64) avgpow_frames_bwd_kernel(const T* __restrict__ yp, long sp, Plan p, const T* __restrict__ w,
                                                               const T* __restrict__ h, const cx<T>* __restrict__ tw,
                                                               const double* __restrict__ keep, T* __restrict__ gframes) {
    __shared__ cx<T> A[ZLDS];
    __shared__ cx<T> Y[NB + 7];
    __shared__ double gQ[IMAX + 6];
    __shared__ double hd[WIN];
    const int lane = threadIdx.x;
    const long f = blockIdx.x;
    hd[lane] = (double)h[lane];
    __syncthreads();
    // dL/dP1 = -(P2 - P1) / (|D| |P1| |P2|) - loss P1 / |P1|^2 (the norm's gradient is 0 at D = 0, as torch's is)
    const double n1 = keep[0], n2 = keep[1], d = keep[2], loss = keep[3];
    const double c1 = d > 0.0 ? -1.0 / (sqrt(d) * sqrt(n1) * sqrt(n2)) : 0.0, c2 = -loss / n1;
    const long n = (long)p.I * p.J;
    const double* p1 = keep + 4;
    const double* p2 = p1 + n;
    // dL/dQ[f][i] = sum_j h[f - sj j] dL/dP1[i][j]
    const long jlo = f >= WIN ? (f - (WIN - 1) + p.sj - 1) / p.sj : 0;
    const long jhi = min((long)p.J - 1, f / p.sj);
    for (int i = lane; i < p.I; i += 64) {
        double acc = 0.0;
        for (long j = jlo; j <= jhi; ++j) {
            const double a1 = p1[j * p.I + i], a2 = p2[j * p.I + i];
            acc += hd[f - p.sj * j] * (c1 * (a2 - a1) + c2 * a1);
        }
        gQ[i] = acc;
    }
    [[clang::always_inline]] framed::frame_transform<T, T, PL, NFFT>(yp, sp, p.T, f, FRAME, w, tw, A, lane);      // (its barriers publish gQ)
    // dL/dS[k] = sum_i h[k - si i] dL/dQ[i]; G = dL/dS X / |X|, halved into the Hermitian spectrum of the inverse transform
    for (int k = lane; k < NB; k += 64) {
        const cx<T> x = framed::split_bin<T, PL, NFFT>(A, tw, k);
        const T mag = hypot(x.x, x.y);
        const int ilo = k >= WIN ? (k - (WIN - 1) + p.si - 1) / p.si : 0;
        const int ihi = min(p.I - 1, k / p.si);
        double gs = 0.0;
        for (int i = ilo; i <= ihi; ++i) gs += hd[k - p.si * i] * gQ[i];
        cx<T> g((T)0, (T)0);
        if (mag > (T)0) g = framed::hermitian_half<T, PL>((T)(gs / (double)mag), x, k);
        Y[k] = g;
    }
    __syncthreads();
    cx<T> v[PL];
#pragma unroll
    for (int r = 0; r < PL; ++r) v[r] = framed::unsplit<T, PL, NFFT>(Y, tw, lane + 64 * r);
    framed::fft_wave<T, PL, NFFT, true>(v, A, tw, lane);
    framed::store_frame_grad<T, T, PL>(A, w, FRAME, gframes + f * NFFT, lane);
}

// ---------------------------------------------------------------- overlap-add: a gather per sample, in a fixed order
template <typename T>
__global__ void __launch_bounds__(256) avgpow_ola_kernel(const T* __restrict__ gframes, Plan p, const T* __restrict__ gloss,
                                                        T* __restrict__ gy) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.T) return;
    // (the gather looks into the right margin for every t <= T - 2; before t = T - 513 the image lies beyond frame `last`
    // and nothing is added)
    double acc = 0.0;
    const bool any = framed::gather_sample(gframes, t, p.T, HALF, FRAME, p.last, acc);
    gy[t] = any ? (T)((double)gloss[0] * acc) : (T)0;
}

}  // namespace avgpow
}  // namespace fl

using namespace fl;
using namespace fl::avgpow;

extern "C" long fl_avgpow_frames(long T) {
    Plan p;
    return make_plan(T, 1, 1, p) ? p.F : -1;
}
extern "C" long fl_avgpow_work_doubles(long T, int si, int sj) {
    Plan p;
    return make_plan(T, si, sj, p) ? 2 * p.F * p.I + 3 * p.nb : -1;
}
extern "C" long fl_avgpow_keep_doubles(long T, int si, int sj) {
    Plan p;
    return make_plan(T, si, sj, p) ? 4 + 2 * (long)p.I * p.J : -1;
}

#define FL_AVGPOW_PLAN(who)                                                                                        \
    Plan p;                                                                                                        \
    FL_REQUIRE(make_plan(Tn, si, sj, p), who ": bad sizes (16128 <= T <= 2^30, strides of the smoothing >= 1)")

// (Tn: the header's T, the signals' length -- T is the precision here)
FL_ENTRY_F32_F64(fl_avgpow_fwd, (const void* yp, long sp, const void* yt, long st, long Tn, int si, int sj, const void* w, const void* h,
                                 const void* tw, void* work, void* keep, void* P1, void* P2, void* loss, void* stream),
                 (yp, sp, yt, st, Tn, si, sj, w, h, tw, work, keep, P1, P2, loss, stream)) {
    FL_REQUIRE(yp && yt && w && h && tw && work && keep && P1 && P2 && loss, "avgpow_fwd: null pointer");
    FL_AVGPOW_PLAN("avgpow_fwd");
    FL_REQUIRE(sp >= 1 && st >= 1, "avgpow_fwd: element strides of the signals must be >= 1");
    FL_REQUIRE((uintptr_t)w % (2 * sizeof(T)) == 0, "avgpow_fwd: the window must be aligned to two of its elements");
    double* Q = (double*)work;
    double* partial = Q + 2 * p.F * p.I;
    hipLaunchKernelGGL((avgpow_frames_kernel<T>), dim3((unsigned)(2 * p.F)), dim3(64), 0, (hipStream_t)stream, (const T*)yp, sp,
                       (const T*)yt, st, p, (const T*)w, (const T*)h, (const cx<T>*)tw, Q);
    FL_CHECK_LAUNCH("avgpow_frames");
    hipLaunchKernelGGL((avgpow_combine_kernel<T>), dim3((unsigned)p.nb), dim3(256), 0, (hipStream_t)stream, (const double*)Q, p,
                       (const T*)h, (double*)keep, (T*)P1, (T*)P2, partial);
    FL_CHECK_LAUNCH("avgpow_combine");
    hipLaunchKernelGGL((avgpow_final_kernel<T>), dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partial, p.nb, (double*)keep,
                       (T*)loss);
    FL_CHECK_LAUNCH("avgpow_final");
    return FL_OK;
}

FL_ENTRY_F32_F64(fl_avgpow_bwd, (const void* yp, long sp, long Tn, int si, int sj, const void* w, const void* h, const void* tw,
                                 const void* keep, const void* gloss, void* gframes, void* gy, void* stream),
                 (yp, sp, Tn, si, sj, w, h, tw, keep, gloss, gframes, gy, stream)) {
    FL_REQUIRE(yp && w && h && tw && keep && gloss && gframes && gy, "avgpow_bwd: null pointer");
    FL_AVGPOW_PLAN("avgpow_bwd");
    FL_REQUIRE(sp >= 1, "avgpow_bwd: the element stride of the signal must be >= 1");
    FL_REQUIRE((uintptr_t)w % (2 * sizeof(T)) == 0 && (uintptr_t)gframes % (2 * sizeof(T)) == 0,
               "avgpow_bwd: the window and the frame gradients must be aligned to two of their elements");
    hipLaunchKernelGGL((avgpow_frames_bwd_kernel<T>), dim3((unsigned)(p.last + 1)), dim3(64), 0, (hipStream_t)stream, (const T*)yp, sp, p,
                       (const T*)w, (const T*)h, (const cx<T>*)tw, (const double*)keep, (T*)gframes);
    FL_CHECK_LAUNCH("avgpow_frames_bwd");
    hipLaunchKernelGGL((avgpow_ola_kernel<T>), dim3((unsigned)((Tn + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const T*)gframes, p,
                       (const T*)gloss, (T*)gy);
    FL_CHECK_LAUNCH("avgpow_ola");
    return FL_OK;
}
