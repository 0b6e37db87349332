// Mel energy-decay-relief criterion (gfx950 / MI355X): of prediction and target the power spectrograms P = |X|^2 of one
// resolution (n_fft, hop, win), their projection on 64 mel bands m = W P, the Schroeder backward integral OVER FRAMES of the
// squared band energies, E[f] = sum_{f' >= f} m[f']^2, in dB, and
//
//   loss = sum |edr_t - edr_p| / sum |edr_t|
//
// over all rows (batch x channel columns), bands and frames at once (include/flamo_hip_edr.h has the definition in full).  In
// torch this is two stft, a matmul, flip / cumsum / flip, two log10, a masked assignment, two norms and the backward of all of
// it.
//
// Launches: THREE forward (frames, relief, final) and THREE backward (prefix, frames, overlap-add), whatever B, N and T.
//
// Frames.  One wavefront per (row, frame) on the framed real transform of framed.h, both signals one after the other.  The
// frame's |X|^2 goes to LDS and lane j sums the taps of band j from there (mel_project of criterion.h, which also states the
// table's format): 64 doubles per frame and signal reach memory, the spectrogram never does.
// The frame length is a template argument here (one resolution per call), so the LDS of a workgroup is that of its n_fft.
//
// Relief.  One workgroup of 16 wavefronts per row, lane = band, so every step of a walk is one coalesced 512-byte load per
// signal.  The frames of the row are cut into 16 consecutive segments; every wavefront first sums m^2 over its segment (last
// frame to first), the segment sums are exchanged through LDS, and the wavefront walks its segment a second time with
// E[f] = (the segments behind it, added last to first) + (its own running sum): only additions of non-negative terms -- E[f]
// is never recovered as E[0] - prefix, which would lose a 60 dB tail (1e-12 of E[0] in squared mel power) -- and E[0], which
// `energy_norm` needs before the first dB value, is known after the exchange, to the bit the walk's value at frame 0.  The
// second walk forms the two dB values, the clip (E_t[f] == 0 exactly: both entries become eps, 0 to the numerator, eps to
// the denominator, no gradient), the row's partial sums and, when a gradient is wanted, sign(edr_t - edr_p) c / E_p[f],
// c = 10 / ln 10, per entry -- with `energy_norm` frame 0 also takes -(c / E_p[0]) sum_f sign.  The final kernel adds the
// rows' sums in a fixed order and writes the loss and 1 / D.
//
// Backward.  dL/dm[f'] = 2 m[f'] sum_{f <= f'} q[f], q = -(kept entry) / D: the prefix kernel is the relief kernel's
// two-walk scan run forward.  The frame kernel recomputes the prediction's transform, gathers dL/dP[k] from the at most two
// (consecutive) bands that hold bin k, forms dL/dX = 2 X dL/dP through the Hermitian split, and runs the adjoint of the
// split and the inverse walk; the overlap-add gathers per sample with the reflected margins folded back.
//
// No atomics (two runs give the same bits), nothing is read back, no allocation depends on the data.
//
// Precision.  As in mrstft.hip: the signals, the frame gradients and the gradient have the signals' type, everything between
// is a double in float32 too.
//
// Resources (the compiler's report for gfx950, n_fft = 2048): LDS A[1088] complex doubles (17 KB) + 1025 doubles of |X|^2
// (8 KB) = 25 KB forward, A + 1025 complex doubles of bins / dL/dX (16 KB) = 33 KB backward, as mrstft.hip's (the frame's 64
// values of dL/dm sit in A between the transform and the inverse walk); the VGPR counts are in DESIGN 4.6; no scratch.
#include "criterion.h"
#include "../../include/flamo_hip_edr.h"

namespace fl {
namespace edr {

using C = double;

constexpr int NFFT_MIN = 256, NFFT_MAX = 2048, NTW = 2048, BANDS = 64;
constexpr long BLOCKS_MAX = (1L << 31) - 1, SAMPLES_MAX = 1L << 38;
constexpr int KEEP_INVD = 0, KEEP_DOUBLES = 1;      // what the backward entry reads again: 1 / D
constexpr int RW = 16;      // wavefronts per row in the relief and prefix kernels

using framed::Strides;
using framed::Mel;      // 64 bands here
using framed::power;
using framed::row_offset;

struct Plan : framed::Frame {
    int nfft;
    long B, T, N, rows, F, blocks;
};

static bool make_plan(long B, long T, long N, int nfft, int hop, int win, Plan& p) {
    if (!framed::signal_sizes(B, T, N, SAMPLES_MAX)) return false;
    if (nfft < NFFT_MIN || nfft > NFFT_MAX || (nfft & (nfft - 1)) || hop < 1 || win < 1 || win > nfft || T <= nfft / 2) return false;
    p.nfft = nfft; p.hop = hop; p.win = win; p.lpad = (nfft - win) / 2;
    p.B = B; p.T = T; p.N = N; p.rows = B * N;
    p.F = framed::frames_per_row(T, hop, p.rows, BLOCKS_MAX);
    if (p.F < 0) return false;
    p.blocks = p.rows * p.F;
    return true;
}

// ---------------------------------------------------------------- forward frames: 64 band energies per frame and signal
template <typename T, int P>
__global__ void __launch_bounds__(64) edr_frames_kernel(const T* __restrict__ yp, Strides sp, const T* __restrict__ yt, Strides st, Plan p,
                                                        const C* __restrict__ w, const cx<C>* __restrict__ tw, Mel mel,
                                                        double* __restrict__ melout) {
    constexpr int NC = 64 * P;
    __shared__ cx<C> A[NC + 64];
    __shared__ double Sp[NC + 1];
    const int lane = threadIdx.x;
    const long row = blockIdx.x / p.F, f = blockIdx.x - row * p.F;
    framed::frame_transform<T, C, P, NTW>(yp + row_offset(p, row, sp), sp.t, p.T, f, p, w, tw, A, lane);
    for (int k = lane; k <= NC; k += 64) Sp[k] = power(framed::split_bin<C, P, NTW>(A, tw, k));
    __syncthreads();
    melout[(long)blockIdx.x * BANDS + lane] = framed::mel_project<64 * P, BANDS>(Sp, mel, lane);
    __syncthreads();
    framed::frame_transform<T, C, P, NTW>(yt + row_offset(p, row, st), st.t, p.T, f, p, w, tw, A, lane);
    for (int k = lane; k <= NC; k += 64) Sp[k] = power(framed::split_bin<C, P, NTW>(A, tw, k));
    __syncthreads();
    melout[(p.blocks + (long)blockIdx.x) * BANDS + lane] = framed::mel_project<64 * P, BANDS>(Sp, mel, lane);
}

// ---------------------------------------------------------------- relief: the backward integral over frames, dB, the row's sums
__global__ void __launch_bounds__(64 * RW) edr_relief_kernel(const double* __restrict__ mel, Plan p, int norm, double eps,
                                                             double* __restrict__ kept, double* __restrict__ rowsum) {
    __shared__ double S[2][RW][BANDS];
    __shared__ double SG[RW][BANDS];
    __shared__ double ND[2][RW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long row = blockIdx.x, F = p.F;
    const long seg = (F + RW - 1) / RW, f0 = min(F, wv * seg), f1 = min(F, f0 + seg);
    const double* mp = mel + row * F * BANDS + lane;
    const double* mt = mp + p.blocks * BANDS;
    double* kp = kept ? kept + row * F * BANDS + lane : nullptr;
    double rp = 0.0, rt = 0.0;
    for (long f = f1 - 1; f >= f0; --f) {
        const double a = mp[f * BANDS], b = mt[f * BANDS];
        rp = fma(a, a, rp);
        rt = fma(b, b, rt);
    }
    S[0][wv][lane] = rp;
    S[1][wv][lane] = rt;
    __syncthreads();
    // the segments behind this one, last to first; carried on to the first, the same chain ends in E[0]
    double tp = 0.0, tt = 0.0, e0p = 0.0, e0t = 0.0;
    for (int v = RW - 1; v >= 0; --v) {
        if (v == wv) {
            tp = e0p;
            tt = e0t;
        }
        e0p += S[0][v][lane];
        e0t += S[1][v][lane];
    }
    const double c = 10.0 / log(10.0);
    double num = 0.0, den = 0.0, sg = 0.0, k0 = 0.0;
    rp = rt = 0.0;
    for (long f = f1 - 1; f >= f0; --f) {
        const double a = mp[f * BANDS], b = mt[f * BANDS];
        rp = fma(a, a, rp);
        rt = fma(b, b, rt);
        const double Ep = tp + rp, Et = tt + rt;
        double k = 0.0;
        if (Et == 0.0) {
            den += eps;
        } else {
            const double ep = 10.0 * log10(norm ? Ep / e0p : Ep), et = 10.0 * log10(norm ? Et / e0t : Et);
            const double d = et - ep;
            const double s = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
            num += fabs(d);
            den += fabs(et);
            sg += s;
            k = s * c / Ep;
        }
        if (kp) kp[f * BANDS] = k;
        if (f == 0) k0 = k;
    }
    num = wave_sum(num);
    den = wave_sum(den);
    if (lane == 0) {
        ND[0][wv] = num;
        ND[1][wv] = den;
    }
    SG[wv][lane] = sg;
    __syncthreads();
    if (wv != 0) return;
    if (norm && kp) {      // d edr[f] / d E[0] = -c / E[0] for every unclipped f
        double tot = 0.0;
        for (int v = 0; v < RW; ++v) tot += SG[v][lane];
        // (a band that is silent in both signals is clipped throughout: tot = 0 and E[0] = 0, and its gradient stays 0)
        if (tot != 0.0) kp[0] = k0 - c / e0p * tot;
    }
    if (lane < 2) {
        double s = 0.0;
        for (int v = 0; v < RW; ++v) s += ND[lane][v];
        rowsum[2 * row + lane] = s;
    }
}

// one wavefront: the rows' sums in a fixed order, the loss and 1 / D
template <typename T>
__global__ void __launch_bounds__(64) edr_final_kernel(const double* __restrict__ rowsum, Plan p, double* __restrict__ keep,
                                                      T* __restrict__ loss) {
    const int lane = threadIdx.x;
    double num = 0.0, den = 0.0;
    for (long r = lane; r < p.rows; r += 64) {
        num += rowsum[2 * r];
        den += rowsum[2 * r + 1];
    }
    num = wave_sum(num);
    den = wave_sum(den);
    if (lane != 0) return;
    keep[KEEP_INVD] = 1.0 / den;
    loss[0] = (T)(num / den);
}

// ---------------------------------------------------------------- backward: dL/dm = 2 m_p (forward prefix sum of q), q = -kept / D
__global__ void __launch_bounds__(64 * RW) edr_prefix_kernel(const double* __restrict__ mel, const double* __restrict__ kept,
                                                             const double* __restrict__ keep, Plan p, double* __restrict__ gmel) {
    __shared__ double S[RW][BANDS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long row = blockIdx.x, F = p.F;
    const long seg = (F + RW - 1) / RW, f0 = min(F, wv * seg), f1 = min(F, f0 + seg);
    const long base = row * F * BANDS + lane;
    const double* mp = mel + base;
    const double* kp = kept + base;
    double* g = gmel + base;
    double r = 0.0;
    for (long f = f0; f < f1; ++f) r += kp[f * BANDS];
    S[wv][lane] = r;
    __syncthreads();
    double head = 0.0;
    for (int v = 0; v < wv; ++v) head += S[v][lane];
    const double scale = -2.0 * keep[KEEP_INVD];
    r = 0.0;
    for (long f = f0; f < f1; ++f) {
        r += kp[f * BANDS];
        g[f * BANDS] = scale * mp[f * BANDS] * (head + r);
    }
}

template <typename T, int P>
__global__ void __launch_bounds__(64) edr_frames_bwd_kernel(const T* __restrict__ yp, Strides sp, Plan p, const C* __restrict__ w,
                                                            const cx<C>* __restrict__ tw, Mel mel, const double* __restrict__ gmel,
                                                            T* __restrict__ gframes) {
    constexpr int NC = 64 * P;
    __shared__ cx<C> A[NC + 64];
    __shared__ cx<C> Y[NC + 1];
    const int lane = threadIdx.x;
    const long row = blockIdx.x / p.F, f = blockIdx.x - row * p.F;
    framed::frame_transform<T, C, P, NTW>(yp + row_offset(p, row, sp), sp.t, p.T, f, p, w, tw, A, lane);
    for (int k = lane; k <= NC; k += 64) Y[k] = framed::split_bin<C, P, NTW>(A, tw, k);
    __syncthreads();
    // the frame's dL/dm in A, free until the inverse walk
    double* G = reinterpret_cast<double*>(A);
    G[lane] = gmel[(long)blockIdx.x * BANDS + lane];
    __syncthreads();
    const int* band = mel.idx + 3 * BANDS;
    const double* bw = mel.w + mel.nnz;
    // dL/dP[k] from the two bands of bin k; G = 2 dL/dP X, halved into the Hermitian spectrum of the inverse transform
    for (int k = lane; k <= NC; k += 64) {
        const int j = min(max(band[k], 0), BANDS - 2);
        const double dP = bw[2 * k] * G[j] + bw[2 * k + 1] * G[j + 1];
        Y[k] = framed::hermitian_half<C, P>(2.0 * dP, Y[k], k);
    }
    __syncthreads();
    cx<C> v[P];
#pragma unroll
    for (int r = 0; r < P; ++r) v[r] = framed::unsplit<C, P, NTW>(Y, tw, lane + 64 * r);
    framed::fft_wave<C, P, NTW, true>(v, A, tw, lane);
    framed::store_frame_grad<T, C, P>(A, w, p, gframes + (long)blockIdx.x * p.win, lane);
}

// overlap-add: a gather per sample, in a fixed order (its own kernel: the plan is the one resolution's Frame itself, not the
// list of them that criterion.h's ola_kernel walks)
template <typename T>
__global__ void __launch_bounds__(256) edr_ola_kernel(const T* __restrict__ gframes, Plan p, const T* __restrict__ gloss, T* __restrict__ gy) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= p.rows * p.T) return;
    const long row = e / p.T, t = e - row * p.T;
    double acc = 0.0;
    framed::gather_sample(gframes + row * p.F * p.win, t, p.T, p.nfft / 2, p, p.F - 1, acc);
    const long b = row / p.N, c = row - b * p.N;
    gy[(b * p.T + t) * p.N + c] = (T)((double)gloss[0] * acc);
}

}  // namespace edr
}  // namespace fl

using namespace fl;
using namespace fl::edr;

extern "C" long fl_edr_frames(long B, long T, long N, int nfft, int hop, int win) {
    Plan p;
    return make_plan(B, T, N, nfft, hop, win, p) ? p.F : -1;
}
extern "C" long fl_edr_band_doubles(long B, long T, long N, int nfft, int hop, int win) {
    Plan p;
    return make_plan(B, T, N, nfft, hop, win, p) ? p.blocks * BANDS : -1;
}
extern "C" long fl_edr_gframe_elems(long B, long T, long N, int nfft, int hop, int win) {
    Plan p;
    return make_plan(B, T, N, nfft, hop, win, p) ? p.blocks * win : -1;
}
extern "C" long fl_edr_keep_doubles(void) { return KEEP_DOUBLES; }
extern "C" long fl_edr_mel_ints(int nfft) { return 3 * BANDS + nfft / 2 + 1; }
extern "C" long fl_edr_mel_doubles(int nfft, int nnz) { return (long)nnz + 2 * (nfft / 2 + 1); }

#define FL_EDR_PLAN(who)                                                                                                        \
    Plan p;                                                                                                                     \
    FL_REQUIRE(make_plan(B, Tn, N, nfft, hop, win, p),                                                                          \
               who ": bad sizes (n_fft a power of two from 256 to 2048, 1 <= win <= n_fft, hop >= 1, n_fft / 2 < T <= 2^30, "   \
                   "fewer than 2^31 frames and at most 2^38 samples in all)");                                                  \
    FL_REQUIRE(nnz >= 0 && nnz <= BANDS * (nfft / 2 + 1), who ": the mel table holds 0 to 64 (n_fft / 2 + 1) weights");          \
    FL_REQUIRE((uintptr_t)tw % (2 * sizeof(C)) == 0, who ": the twiddle table must be aligned to its complex elements")

// (Tn: the header's T, the signals' length -- T is the precision here)
FL_ENTRY_F32_F64(fl_edr_fwd, (const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long Tn,
                              long N, int nfft, int hop, int win, const void* wtab, const void* tw, const void* melidx, const void* melw,
                              int nnz, int energy_norm, double eps, void* mel, void* kept, void* rowsum, void* keep, void* loss,
                              void* stream),
                 (yp, spb, spt, spc, yt, stb, stt, stc, B, Tn, N, nfft, hop, win, wtab, tw, melidx, melw, nnz, energy_norm, eps, mel, kept,
                  rowsum, keep, loss, stream)) {
    FL_REQUIRE(yp && yt && wtab && tw && melidx && melw && mel && rowsum && keep && loss, "edr_fwd: null pointer");
    FL_EDR_PLAN("edr_fwd");
    FL_REQUIRE(eps >= 0.0, "edr_fwd: eps must be >= 0");
    const Mel m{(const int*)melidx, (const double*)melw, nnz};
    const Strides sp{spb, spt, spc}, st{stb, stt, stc};
    dispatch<2, 4, 8, 16>(nfft / 128, [&](auto Pc) {
        hipLaunchKernelGGL((edr_frames_kernel<T, decltype(Pc)::value>), dim3((unsigned)p.blocks), dim3(64), 0, (hipStream_t)stream,
                           (const T*)yp, sp, (const T*)yt, st, p, (const C*)wtab, (const cx<C>*)tw, m, (double*)mel);
    });
    FL_CHECK_LAUNCH("edr_frames");
    hipLaunchKernelGGL(edr_relief_kernel, dim3((unsigned)p.rows), dim3(64 * RW), 0, (hipStream_t)stream, (const double*)mel, p,
                       energy_norm ? 1 : 0, eps, (double*)kept, (double*)rowsum);
    FL_CHECK_LAUNCH("edr_relief");
    hipLaunchKernelGGL((edr_final_kernel<T>), dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)rowsum, p, (double*)keep,
                       (T*)loss);
    FL_CHECK_LAUNCH("edr_final");
    return FL_OK;
}

FL_ENTRY_F32_F64(fl_edr_bwd, (const void* yp, long spb, long spt, long spc, long B, long Tn, long N, int nfft, int hop, int win,
                              const void* wtab, const void* tw, const void* melidx, const void* melw, int nnz, const void* mel,
                              const void* kept, const void* keep, const void* gloss, void* gmel, void* gframes, void* gy, void* stream),
                 (yp, spb, spt, spc, B, Tn, N, nfft, hop, win, wtab, tw, melidx, melw, nnz, mel, kept, keep, gloss, gmel, gframes, gy,
                  stream)) {
    FL_REQUIRE(yp && wtab && tw && melidx && melw && mel && kept && keep && gloss && gmel && gframes && gy, "edr_bwd: null pointer");
    FL_EDR_PLAN("edr_bwd");
    const Mel m{(const int*)melidx, (const double*)melw, nnz};
    hipLaunchKernelGGL(edr_prefix_kernel, dim3((unsigned)p.rows), dim3(64 * RW), 0, (hipStream_t)stream, (const double*)mel,
                       (const double*)kept, (const double*)keep, p, (double*)gmel);
    FL_CHECK_LAUNCH("edr_prefix");
    dispatch<2, 4, 8, 16>(nfft / 128, [&](auto Pc) {
        hipLaunchKernelGGL((edr_frames_bwd_kernel<T, decltype(Pc)::value>), dim3((unsigned)p.blocks), dim3(64), 0, (hipStream_t)stream,
                           (const T*)yp, Strides{spb, spt, spc}, p, (const C*)wtab, (const cx<C>*)tw, m, (const double*)gmel,
                           (T*)gframes);
    });
    FL_CHECK_LAUNCH("edr_frames_bwd");
    const long blocks = (p.rows * p.T + 255) / 256;
    hipLaunchKernelGGL((edr_ola_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const T*)gframes, p,
                       (const T*)gloss, (T*)gy);
    FL_CHECK_LAUNCH("edr_ola");
    return FL_OK;
}
