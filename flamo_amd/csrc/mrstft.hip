// Multi-resolution STFT criterion (gfx950 / MI355X): for each resolution (n_fft, hop, win) the magnitude spectrograms of
// prediction and target, M = sqrt(max(|X|^2, eps)), and of them
//
//   sc = |M_t - M_p|_F / |M_t|_F      log = mean |log M_p - log M_t|      lin = mean |M_p - M_t|
//
// over all rows (batch x channel columns), bins and frames; the loss is the mean over the resolutions of the weighted three
// (include/flamo_hip_mrstft.h has the definition in full).  In torch this is, per resolution, two stft, clamp, sqrt, two log,
// three reductions and the backward of all of it.
//
// Launches: THREE forward (frames, combine, final) and TWO backward (frames, overlap-add), for all resolutions, rows and both
// signals together, whatever the number of resolutions: the frame kernels' grid is the list of all (resolution, row, frame)
// triples, and the frame length is uniform per workgroup.
//
// Frames.  One wavefront per frame on the framed real transform of framed.h (the packed Stockham walk, its LDS padding and
// register budget, the split into bins and its adjoint are described there), P = n_fft / 128 = 2, 4, 8, 16 complex values per
// lane.  The spectrograms never reach memory: a frame leaves four doubles (sum (M_t - M_p)^2, sum M_t^2,
// sum |log M_p - log M_t|, sum |M_p - M_t|), the combine of criterion.h adds them per resolution in a fixed order (no atomics:
// two runs give the same bits), the final kernel forms the loss and the three factors of dL/dM_p the backward pass needs.  The
// backward frame kernel recomputes both transforms, forms dL/dX = dL/dM_p X / M_p (zero where |X|^2 <= eps), runs the adjoint
// of the split and the inverse walk, and writes the win samples under the window; the overlap-add of criterion.h gathers per
// sample, resolution by resolution and frame by frame, with the reflected margins folded back onto the samples they mirror.
//
// Precision.  The signals, the frame gradients and the gradient have the signals' type; everything between is a double in
// float32 too (see `C` below), so the two precisions run the same kernels and differ in their loads and stores.
//
// LDS.  The walk's A[Nc + 64] complex doubles, sized for n_fft = 2048: 1088 values, 17 KB.  Beside it the forward kernel keeps
// the prediction's clamped |X|^2 (1025 doubles, 8 KB) and the backward kernel the prediction's bins, then dL/dX (1025 complex
// doubles, 16 KB): 25 KB forward and 33 KB backward per wavefront, six and four wavefronts per CU of its 160 KB.  The
// compiler reports 170 VGPRs for the forward and 200 for the backward kernel, no scratch: at four to six wavefronts per CU it
// is LDS, not registers, that bounds the occupancy.
#include "criterion.h"
#include "../../include/flamo_hip_mrstft.h"

namespace fl {
namespace mrstft {

// Everything between the loads of the signals and the stores of the gradient is a double, in float32 too: a float32 transform
// leaves an absolute error of ~6e-8 |frame| on every bin, and the log term weighs a bin by 1 / M^2 -- on decaying responses the
// quiet bins then carry a relative error thousands of roundoffs large into the gradient (as the float32 torch lines do).
using C = double;

constexpr int MAXR = 8, NFFT_MIN = 256, NFFT_MAX = 2048, NTW = 2048;
constexpr int NC_MAX = NFFT_MAX / 2, ALDS = NC_MAX + 64, NB_MAX = NC_MAX + 1;
constexpr long BLOCKS_MAX = (1L << 31) - 1, SAMPLES_MAX = 1L << 38;
constexpr int KEEP_STRIDE = 8, KEEP_LOSS = KEEP_STRIDE * MAXR, KEEP_DOUBLES = KEEP_LOSS + 1;

using framed::Strides;
using framed::power;
using framed::row_offset;

struct Res : framed::Frame {
    int nfft;
    long F;        // frames per row
    long blk0;     // first workgroup of the frame kernels
    long g0;       // first element in gframes
    long w0;       // first element in the window table
};
struct Plan {
    int R;
    long B, T, N, rows, blocks, gelems;
    Res r[MAXR];
};

static bool make_plan(long B, long T, long N, int R, const int* res, Plan& p) {
    if (!res || R < 1 || R > MAXR || !framed::signal_sizes(B, T, N, SAMPLES_MAX)) return false;
    p.R = R; p.B = B; p.T = T; p.N = N; p.rows = B * N;
    long blocks = 0, g = 0, w = 0;
    for (int r = 0; r < R; ++r) {
        const int nfft = res[3 * r], hop = res[3 * r + 1], win = res[3 * r + 2];
        if (nfft < NFFT_MIN || nfft > NFFT_MAX || (nfft & (nfft - 1)) || hop < 1 || win < 1 || win > nfft || T <= nfft / 2) return false;
        Res& q = p.r[r];
        q.nfft = nfft; q.hop = hop; q.win = win; q.lpad = (nfft - win) / 2;
        q.F = framed::frames_per_row(T, hop, p.rows, BLOCKS_MAX);
        if (q.F < 0) return false;
        q.blk0 = blocks; q.g0 = g; q.w0 = w;
        blocks += p.rows * q.F;
        if (blocks > BLOCKS_MAX) return false;
        g += p.rows * q.F * win;
        w += win;
    }
    p.blocks = blocks; p.gelems = g;
    return true;
}

// (resolution, row, frame) of a workgroup
__device__ inline void locate(const Plan& p, long blk, int& r, long& row, long& f) {
    r = p.R - 1;
    while (r > 0 && blk < p.r[r].blk0) --r;
    const long local = blk - p.r[r].blk0;
    row = local / p.r[r].F;
    f = local - row * p.r[r].F;
}

// ---------------------------------------------------------------- forward: the four sums of a frame
template <typename T, int P>
__device__ inline void frame_sums(const T* __restrict__ yp, long sp, const T* __restrict__ yt, long st, long Tn, long f, const Res& q,
                                  const C* __restrict__ w, const cx<C>* __restrict__ tw, double eps, cx<C>* A, double* Sp,
                                  double* __restrict__ out, int lane) {
    constexpr int NC = 64 * P;
    framed::frame_transform<T, C, P, NTW>(yp, sp, Tn, f, q, w, tw, A, lane);
    for (int k = lane; k <= NC; k += 64) Sp[k] = fmax(power(framed::split_bin<C, P, NTW>(A, tw, k)), eps);
    __syncthreads();
    framed::frame_transform<T, C, P, NTW>(yt, st, Tn, f, q, w, tw, A, lane);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int k = lane; k <= NC; k += 64) {
        const double pt = fmax(power(framed::split_bin<C, P, NTW>(A, tw, k)), eps), pp = Sp[k];
        const double mp = sqrt(pp), mt = sqrt(pt), d = mt - mp;
        s0 += d * d;
        s1 += mt * mt;
        s2 += fabs(0.5 * (log(pp) - log(pt)));
        s3 += fabs(d);
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    s3 = wave_sum(s3);
    if (lane == 0) {
        out[0] = s0;
        out[1] = s1;
        out[2] = s2;
        out[3] = s3;
    }
}

template <typename T>
__global__ void __launch_bounds__(64) mrstft_frames_kernel(const T* __restrict__ yp, Strides sp, const T* __restrict__ yt, Strides st,
                                                           Plan p, const C* __restrict__ wtab, const cx<C>* __restrict__ tw,
                                                           double eps, double* __restrict__ partial) {
    __shared__ cx<C> A[ALDS];
    __shared__ double Sp[NB_MAX];
    const int lane = threadIdx.x;
    int r;
    long row, f;
    locate(p, blockIdx.x, r, row, f);
    const Res& q = p.r[r];
    const T* a = yp + row_offset(p, row, sp);
    const T* b = yt + row_offset(p, row, st);
    const C* w = wtab + q.w0;
    double* out = partial + 4 * (long)blockIdx.x;
    switch (q.nfft) {
        case 256: frame_sums<T, 2>(a, sp.t, b, st.t, p.T, f, q, w, tw, eps, A, Sp, out, lane); break;
        case 512: frame_sums<T, 4>(a, sp.t, b, st.t, p.T, f, q, w, tw, eps, A, Sp, out, lane); break;
        case 1024: frame_sums<T, 8>(a, sp.t, b, st.t, p.T, f, q, w, tw, eps, A, Sp, out, lane); break;
        default: frame_sums<T, 16>(a, sp.t, b, st.t, p.T, f, q, w, tw, eps, A, Sp, out, lane); break;
    }
}

// one thread: the loss and, per resolution, the factors of dL/dM_p = c0 (M_p - M_t) + c1 sign / M_p + c2 sign
// (the norm's gradient is 0 at M_p = M_t, as torch's is)
template <typename T>
__global__ void __launch_bounds__(64) mrstft_final_kernel(Plan p, double w_sc, double w_log, double w_lin, double* __restrict__ keep,
                                                         T* __restrict__ loss) {
    if (threadIdx.x != 0) return;
    double l = 0.0;
    for (int r = 0; r < p.R; ++r) {
        double* k = keep + KEEP_STRIDE * r;
        const double n = (double)p.rows * (double)p.r[r].F * (double)(p.r[r].nfft / 2 + 1);
        const double D = k[0], S = k[1];
        l += w_sc * (sqrt(D) / sqrt(S)) + w_log * (k[2] / n) + w_lin * (k[3] / n);
        k[4] = D > 0.0 ? w_sc / (p.R * sqrt(D) * sqrt(S)) : 0.0;
        k[5] = w_log / (p.R * n);
        k[6] = w_lin / (p.R * n);
        k[7] = 0.0;
    }
    l /= p.R;
    keep[KEEP_LOSS] = l;
    loss[0] = (T)l;
}

// ---------------------------------------------------------------- backward: the gradient of a frame's windowed samples
template <typename T, int P>
__device__ inline void frame_grad(const T* __restrict__ yp, long sp, const T* __restrict__ yt, long st, long Tn, long f, const Res& q,
                                  const C* __restrict__ w, const cx<C>* __restrict__ tw, double eps, const double* __restrict__ coef,
                                  cx<C>* A, cx<C>* Y, T* __restrict__ out, int lane) {
    constexpr int NC = 64 * P;
    const double c0 = coef[4], c1 = coef[5], c2 = coef[6];
    framed::frame_transform<T, C, P, NTW>(yp, sp, Tn, f, q, w, tw, A, lane);
    for (int k = lane; k <= NC; k += 64) Y[k] = framed::split_bin<C, P, NTW>(A, tw, k);
    __syncthreads();
    framed::frame_transform<T, C, P, NTW>(yt, st, Tn, f, q, w, tw, A, lane);
    // G = dL/dM_p X / M_p, halved into the Hermitian spectrum of the inverse transform
    for (int k = lane; k <= NC; k += 64) {
        const cx<C> x = Y[k];
        const double pp = power(x);
        cx<C> g(0.0, 0.0);
        if (pp > eps) {
            const double pt = fmax(power(framed::split_bin<C, P, NTW>(A, tw, k)), eps);
            const double mp = sqrt(pp), mt = sqrt(pt);
            const double sg = pp > pt ? 1.0 : (pp < pt ? -1.0 : 0.0);
            const double s = (c0 * (mp - mt) + c1 * sg / mp + c2 * sg) / mp;
            g = framed::hermitian_half<C, P>(s, x, k);
        }
        Y[k] = g;
    }
    __syncthreads();
    cx<C> v[P];
#pragma unroll
    for (int r = 0; r < P; ++r) v[r] = framed::unsplit<C, P, NTW>(Y, tw, lane + 64 * r);
    framed::fft_wave<C, P, NTW, true>(v, A, tw, lane);
    framed::store_frame_grad<T, C, P>(A, w, q, out, lane);
}

template <typename T>
__global__ void __launch_bounds__(64) mrstft_frames_bwd_kernel(const T* __restrict__ yp, Strides sp, const T* __restrict__ yt, Strides st,
                                                               Plan p, const C* __restrict__ wtab, const cx<C>* __restrict__ tw,
                                                               double eps, const double* __restrict__ keep, T* __restrict__ gframes) {
    __shared__ cx<C> A[ALDS];
    __shared__ cx<C> Y[NB_MAX];
    const int lane = threadIdx.x;
    int r;
    long row, f;
    locate(p, blockIdx.x, r, row, f);
    const Res& q = p.r[r];
    const T* a = yp + row_offset(p, row, sp);
    const T* b = yt + row_offset(p, row, st);
    const C* w = wtab + q.w0;
    const double* coef = keep + KEEP_STRIDE * r;
    T* out = gframes + q.g0 + (row * q.F + f) * q.win;
    switch (q.nfft) {
        case 256: frame_grad<T, 2>(a, sp.t, b, st.t, p.T, f, q, w, tw, eps, coef, A, Y, out, lane); break;
        case 512: frame_grad<T, 4>(a, sp.t, b, st.t, p.T, f, q, w, tw, eps, coef, A, Y, out, lane); break;
        case 1024: frame_grad<T, 8>(a, sp.t, b, st.t, p.T, f, q, w, tw, eps, coef, A, Y, out, lane); break;
        default: frame_grad<T, 16>(a, sp.t, b, st.t, p.T, f, q, w, tw, eps, coef, A, Y, out, lane); break;
    }
}

}  // namespace mrstft
}  // namespace fl

using namespace fl;
using namespace fl::mrstft;

extern "C" long fl_mrstft_blocks(long B, long T, long N, int R, int* res) {
    Plan p;
    return make_plan(B, T, N, R, res, p) ? p.blocks : -1;
}
extern "C" long fl_mrstft_gframe_elems(long B, long T, long N, int R, int* res) {
    Plan p;
    return make_plan(B, T, N, R, res, p) ? p.gelems : -1;
}
extern "C" long fl_mrstft_keep_doubles(void) { return KEEP_DOUBLES; }

#define FL_MRSTFT_PLAN(who)                                                                                                  \
    Plan p;                                                                                                                  \
    FL_REQUIRE(make_plan(B, Tn, N, R, res, p),                                                                               \
               who ": bad sizes (1 <= R <= 8 resolutions, n_fft a power of two from 256 to 2048, 1 <= win <= n_fft, hop >= 1, " \
                   "n_fft / 2 < T <= 2^30, fewer than 2^31 frames and at most 2^38 samples in all)")

// (Tn: the header's T, the signals' length -- T is the precision here)
FL_ENTRY_F32_F64(fl_mrstft_fwd, (const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long Tn,
                                 long N, int R, int* res, const void* wtab, const void* tw, double w_sc, double w_log, double w_lin,
                                 double eps, void* partial, void* keep, void* loss, void* stream),
                 (yp, spb, spt, spc, yt, stb, stt, stc, B, Tn, N, R, res, wtab, tw, w_sc, w_log, w_lin, eps, partial, keep, loss, stream)) {
    FL_REQUIRE(yp && yt && res && wtab && tw && partial && keep && loss, "mrstft_fwd: null pointer");
    FL_MRSTFT_PLAN("mrstft_fwd");
    FL_REQUIRE(eps >= 0.0, "mrstft_fwd: eps must be >= 0");
    FL_REQUIRE((uintptr_t)tw % (2 * sizeof(C)) == 0, "mrstft_fwd: the twiddle table must be aligned to its complex elements");
    hipLaunchKernelGGL((mrstft_frames_kernel<T>), dim3((unsigned)p.blocks), dim3(64), 0, (hipStream_t)stream, (const T*)yp,
                       Strides{spb, spt, spc}, (const T*)yt, Strides{stb, stt, stc}, p, (const C*)wtab, (const cx<C>*)tw, eps,
                       (double*)partial);
    FL_CHECK_LAUNCH("mrstft_frames");
    const framed::Spans sums = framed::spans_of(p, [](const Res& q) { return q.blk0; }, [&](const Res& q) { return p.rows * q.F; });
    hipLaunchKernelGGL((framed::combine_kernel<4, KEEP_STRIDE>), dim3((unsigned)p.R), dim3(256), 0, (hipStream_t)stream,
                       (const double*)partial, sums, (double*)keep);
    FL_CHECK_LAUNCH("mrstft_combine");
    hipLaunchKernelGGL((mrstft_final_kernel<T>), dim3(1), dim3(64), 0, (hipStream_t)stream, p, w_sc, w_log, w_lin, (double*)keep,
                       (T*)loss);
    FL_CHECK_LAUNCH("mrstft_final");
    return FL_OK;
}

FL_ENTRY_F32_F64(fl_mrstft_bwd, (const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long Tn,
                                 long N, int R, int* res, const void* wtab, const void* tw, double eps, const void* keep,
                                 const void* gloss, void* gframes, void* gy, void* stream),
                 (yp, spb, spt, spc, yt, stb, stt, stc, B, Tn, N, R, res, wtab, tw, eps, keep, gloss, gframes, gy, stream)) {
    FL_REQUIRE(yp && yt && res && wtab && tw && keep && gloss && gframes && gy, "mrstft_bwd: null pointer");
    FL_MRSTFT_PLAN("mrstft_bwd");
    FL_REQUIRE(eps >= 0.0, "mrstft_bwd: eps must be >= 0");
    FL_REQUIRE((uintptr_t)tw % (2 * sizeof(C)) == 0, "mrstft_bwd: the twiddle table must be aligned to its complex elements");
    hipLaunchKernelGGL((mrstft_frames_bwd_kernel<T>), dim3((unsigned)p.blocks), dim3(64), 0, (hipStream_t)stream, (const T*)yp,
                       Strides{spb, spt, spc}, (const T*)yt, Strides{stb, stt, stc}, p, (const C*)wtab, (const cx<C>*)tw, eps,
                       (const double*)keep, (T*)gframes);
    FL_CHECK_LAUNCH("mrstft_frames_bwd");
    const long blocks = (p.rows * p.T + 255) / 256;
    hipLaunchKernelGGL((framed::ola_kernel<T, Plan>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const T*)gframes, p,
                       (const T*)gloss, (T*)gy);
    FL_CHECK_LAUNCH("mrstft_ola");
    return FL_OK;
}
