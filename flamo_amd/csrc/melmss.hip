// Mel multi-scale spectral criterion (gfx950 / MI355X): for each resolution n_fft (hop = its share of n_fft, the window the
// periodic Hann of n_fft samples) the power spectrograms P = |X|^2 of prediction and target, their projection on n_fft / 8
// mel bands m = W P, a mask from the target's signal-to-noise ratio, and
//
//   |(m_t - m_p) mask| / Nn  +  alpha |(log m_t - log m_p) mask| / Nn        (the second term with log_term)
//
// over all rows (batch x channel columns), bands and frames at once, |.| the Frobenius or the 1-norm, Nn the sum of the mask;
// the loss is the SUM over the resolutions (include/flamo_hip_melmss.h has the definition in full).  In torch this is, per
// resolution, two stft, two dense matmuls, the mask, two to four logs, the norms and the backward of all of it.
//
// Launches: at most FOUR forward (frames of the short resolutions, frames of the long ones, combine, final) and at most THREE
// backward (the same two frame launches, overlap-add), whatever B, N, T and the data: the count depends on the list of
// n_fft alone (a size class without a resolution is not launched; fl_melmss_launches says the number).
//
// Two size classes.  The LDS of a 4096 frame is 49 KB forward and 66 KB backward; one grid sized for it would hold the 128 ..
// 1024 frames, which need 13 and 17 KB, to a third of their occupancy.  So the resolutions with n_fft <= 1024 run in one
// launch of one wavefront per frame (the three-pass walk of framed.h, P = 1, 2, 4, 8 complex values per lane), and those with
// n_fft > 1024 in a second launch of four wavefronts per frame (the wide four-pass walk of framed.h, P = 16, 32: one radix-8
// butterfly per thread and pass).  Each grid is the list of its class's (resolution, row, frame) triples, the longest frames
// first.
//
// Forward frames.  Both signals one after the other: the frame's |X|^2 goes to LDS and thread j sums the taps of the bands j,
// j + (threads), ... from there (mel_project of criterion.h, which also states the table's format).  The prediction's band
// energies wait in registers (two per thread at most) for the target's; a frame leaves five doubles, sum mask d^2, sum mask
// |d|, the same two of the log difference and sum mask -- the mel spectrograms never reach memory.  The combine of
// criterion.h adds them per resolution in a fixed order (no atomics: two runs give the same bits), the final kernel forms the
// loss and the two factors of dL/dm_p per resolution.
//
// Backward frames.  Both transforms are recomputed, the target's first: a signal's bins go to Y, their |X|^2 into the walk's
// array (free between a transform and the next walk), the band energies to registers; after the second pass Y holds the
// prediction's bins.  dL/dm_p is formed per band and laid beside the |X|^2; dL/dP[k] is gathered from the at most two
// (consecutive) bands that hold bin k, dL/dX = 2 X dL/dP through the Hermitian split, the adjoint of the split, the inverse
// walk and the windowed store.  The overlap-add of criterion.h gathers per sample, resolution by resolution, with the
// reflected margins folded back.
//
// In both frame kernels the two signals run through ONE loop body (`both_signals` of criterion.h), so that a prediction equal
// to the target gives band energies equal to the bit, and with them an exact 0 for the loss and for sign(m_t - m_p).
//
// Precision.  As in mrstft.hip and edr.hip: the signals, the frame gradients and the gradient have the signals' type,
// everything between is a double in float32 too -- the mask decision and the signs of the 1-norm are those of the float64
// statement.
//
// Resources (the compiler's report for gfx950 is in DESIGN 4.6): LDS forward A + |X|^2 = 9 + 4 KB (short) and 33 + 16 KB
// (long), backward A + Y = 9 + 8 KB and 33 + 32 KB; no scratch.
#include "criterion.h"
#include "../../include/flamo_hip_melmss.h"

namespace fl {
namespace melmss {

using C = double;

constexpr int MAXR = 8, NFFT_MIN = 128, NFFT_SHORT = 1024, NFFT_MAX = 4096, NTW = 4096;
constexpr int NT_SHORT = 64, NT_LONG = framed::WIDE_NT;
constexpr long BLOCKS_MAX = (1L << 31) - 1, SAMPLES_MAX = 1L << 38;
constexpr int NSUM = 5;      // sum mask d^2, sum mask |d|, the same two of the log difference, sum mask
constexpr int KEEP_STRIDE = 8, KEEP_C0 = 5, KEEP_C1 = 6, KEEP_LOSS = KEEP_STRIDE * MAXR, KEEP_DOUBLES = KEEP_LOSS + 1;

using framed::Strides;
using framed::Mel;      // of one resolution, n_fft / 8 bands
using framed::power;
using framed::sign;
using framed::row_offset;
using framed::snr_mask;
using framed::both_signals;

struct Res : framed::Frame {
    int nfft, nnz;
    long F;        // frames per row
    long blk0;     // first workgroup in the frame kernels of its size class
    long fr0;      // first frame in `partial`
    long g0;       // first element in gframes
    long w0;       // first element in the window table
    long mi0;      // first int in melidx
    long mw0;      // first double in melw
};
struct Plan {
    int R;
    long B, T, N, rows, frames, gelems, blocks[2], melints, meldoubles;
    Res r[MAXR];
};
struct Opt {
    int norm, log_term, apply_mask;
    double alpha, threshold, ne;
};

static bool is_long(int nfft) { return nfft > NFFT_SHORT; }

// the part of a plan that the list of resolutions alone decides
static bool make_tables(int R, const int* res, Plan& p) {
    if (!res || R < 1 || R > MAXR) return false;
    p.R = R;
    long w = 0, mi = 0, mw = 0;
    for (int r = 0; r < R; ++r) {
        const int nfft = res[3 * r], hop = res[3 * r + 1], nnz = res[3 * r + 2];
        if (nfft < NFFT_MIN || nfft > NFFT_MAX || (nfft & (nfft - 1)) || hop < 1) return false;
        if (nnz < 0 || nnz > (nfft / 8) * (nfft / 2 + 1)) return false;
        Res& q = p.r[r];
        q.nfft = nfft; q.hop = hop; q.win = nfft; q.lpad = 0; q.nnz = nnz;
        q.w0 = w; q.mi0 = mi; q.mw0 = mw;
        w += nfft;
        mi += 3 * (nfft / 8) + nfft / 2 + 1;
        mw += (long)nnz + 2 * (nfft / 2 + 1);
    }
    p.melints = mi; p.meldoubles = mw;
    return true;
}

static bool make_plan(long B, long T, long N, int R, const int* res, Plan& p) {
    if (!make_tables(R, res, p) || !framed::signal_sizes(B, T, N, SAMPLES_MAX)) return false;
    p.B = B; p.T = T; p.N = N; p.rows = B * N;
    long frames = 0, g = 0;
    for (int r = 0; r < R; ++r) {
        Res& q = p.r[r];
        if (T <= q.nfft / 2) return false;
        q.F = framed::frames_per_row(T, q.hop, p.rows, BLOCKS_MAX);
        if (q.F < 0) return false;
        q.fr0 = frames; q.g0 = g;
        frames += p.rows * q.F;
        if (frames > BLOCKS_MAX) return false;
        g += p.rows * q.F * q.nfft;
    }
    // the workgroups of a size class, longest frames first: a frame of 1024 takes several times as long as one of 128, and
    // started behind the 3001 short frames of a row it would be the tail of the launch
    p.blocks[0] = p.blocks[1] = 0;
    for (int nfft = NFFT_MAX; nfft >= NFFT_MIN; nfft /= 2)
        for (int r = 0; r < R; ++r) {
            Res& q = p.r[r];
            if (q.nfft != nfft) continue;
            long& blocks = p.blocks[is_long(nfft)];
            q.blk0 = blocks;
            blocks += p.rows * q.F;
        }
    p.frames = frames; p.gelems = g;
    return true;
}

// (resolution, row, frame) of a workgroup of the size class LONG: the resolution of the class that starts last at or before it
template <bool LONG>
__device__ inline void locate(const Plan& p, long blk, int& r, long& row, long& f) {
    r = 0;
    long best = -1;
    for (int i = 0; i < p.R; ++i)
        if ((p.r[i].nfft > NFFT_SHORT) == LONG && blk >= p.r[i].blk0 && p.r[i].blk0 > best) {
            r = i;
            best = p.r[i].blk0;
        }
    const long local = blk - p.r[r].blk0;
    row = local / p.r[r].F;
    f = local - row * p.r[r].F;
}

template <int P> struct Shape {
    static constexpr bool LONG = P >= 16;
    static constexpr int NC = 64 * P, NT = LONG ? NT_LONG : NT_SHORT, NM = 16 * P;      // bins - 1, threads, bands
    static constexpr int NB = NM > NT ? NM / NT : 1;                                     // bands per thread
};

template <typename T, int P>
__device__ inline void transform(const T* __restrict__ y, long stride, long Tn, long f, const Res& q, const C* __restrict__ w,
                                 const cx<C>* __restrict__ tw, cx<C>* A, int tid) {
    if constexpr (Shape<P>::LONG) framed::frame_transform_wide<T, C, P, NTW>(y, stride, Tn, f, q, w, tw, A, tid);
    else framed::frame_transform<T, C, P, NTW>(y, stride, Tn, f, q, w, tw, A, tid);
}

// ---------------------------------------------------------------- forward: the five sums of a frame
template <typename T, int P>
__device__ inline void frame_sums(const T* __restrict__ yp, long sp, const T* __restrict__ yt, long st, long Tn, long f, const Res& q,
                                  const C* __restrict__ w, const cx<C>* __restrict__ tw, const Mel& mel, const Opt& o, cx<C>* A,
                                  double* Sp, double (*red)[4], double* __restrict__ out, int tid) {
    constexpr int NC = Shape<P>::NC, NT = Shape<P>::NT, NM = Shape<P>::NM, NB = Shape<P>::NB;
    // one body for both signals (see the note at `both_signals`, criterion.h): the prediction, then the target
    double mp[NB], mt[NB];
    both_signals<NB>(mp, mt, [&](int sig, double (&m)[NB]) {
        transform<T, P>(sig ? yt : yp, sig ? st : sp, Tn, f, q, w, tw, A, tid);
        for (int k = tid; k <= NC; k += NT) Sp[k] = power(framed::split_bin<C, P, NTW>(A, tw, k));
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NB; ++i) m[i] = tid + NT * i < NM ? framed::mel_project<NC, NM>(Sp, mel, tid + NT * i) : 0.0;
        __syncthreads();
    });
    double s[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int j = tid + NT * i;
        if (j < NM) {
            const double mask = snr_mask(mt[i], o);
            const double d = (mt[i] - mp[i]) * mask;
            s[0] += d * d;
            s[1] += fabs(d);
            if (o.log_term) {
                const double dl = (log(mt[i]) - log(mp[i])) * mask;
                s[2] += dl * dl;
                s[3] += fabs(dl);
            }
            s[4] += mask;
        }
    }
#pragma unroll
    for (int c = 0; c < NSUM; ++c) s[c] = wave_sum(s[c]);
    if constexpr (NT == 64) {
        if (tid == 0) {
#pragma unroll
            for (int c = 0; c < NSUM; ++c) out[c] = s[c];
        }
    } else {
        if ((tid & 63) == 0) {
#pragma unroll
            for (int c = 0; c < NSUM; ++c) red[c][tid >> 6] = s[c];
        }
        __syncthreads();
        if (tid < NSUM) out[tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
    }
}

template <typename T, bool LONG>
__global__ void __launch_bounds__(LONG ? NT_LONG : NT_SHORT)
melmss_frames_kernel(const T* __restrict__ yp, Strides sp, const T* __restrict__ yt, Strides st, Plan p, const C* __restrict__ wtab,
                     const cx<C>* __restrict__ tw, const int* __restrict__ melidx, const double* __restrict__ melw, Opt o,
                     double* __restrict__ partial) {
    constexpr int NC_MAX = (LONG ? NFFT_MAX : NFFT_SHORT) / 2;
    __shared__ cx<C> A[NC_MAX + 64];
    __shared__ double Sp[NC_MAX + 1];
    __shared__ double red[NSUM][4];
    const int tid = threadIdx.x;
    int r;
    long row, f;
    locate<LONG>(p, blockIdx.x, r, row, f);
    const Res& q = p.r[r];
    const T* a = yp + row_offset(p, row, sp);
    const T* b = yt + row_offset(p, row, st);
    const C* w = wtab + q.w0;
    const Mel mel{melidx + q.mi0, melw + q.mw0, q.nnz};
    double* out = partial + NSUM * (q.fr0 + row * q.F + f);
    if constexpr (LONG) {
        if (q.nfft == 2048) frame_sums<T, 16>(a, sp.t, b, st.t, p.T, f, q, w, tw, mel, o, A, Sp, red, out, tid);
        else frame_sums<T, 32>(a, sp.t, b, st.t, p.T, f, q, w, tw, mel, o, A, Sp, red, out, tid);
    } else {
        switch (q.nfft) {
            case 128: frame_sums<T, 1>(a, sp.t, b, st.t, p.T, f, q, w, tw, mel, o, A, Sp, red, out, tid); break;
            case 256: frame_sums<T, 2>(a, sp.t, b, st.t, p.T, f, q, w, tw, mel, o, A, Sp, red, out, tid); break;
            case 512: frame_sums<T, 4>(a, sp.t, b, st.t, p.T, f, q, w, tw, mel, o, A, Sp, red, out, tid); break;
            default: frame_sums<T, 8>(a, sp.t, b, st.t, p.T, f, q, w, tw, mel, o, A, Sp, red, out, tid); break;
        }
    }
}

// one thread: the loss and, per resolution, the factors of dL/dm_p = -mask (c0 d + c1 dl / m_p) (norm 2; the norm's
// gradient is 0 where the norm is, as torch's is) or -mask (c0 sign d + c1 sign dl / m_p) (norm 1)
template <typename T>
__global__ void __launch_bounds__(64) melmss_final_kernel(Plan p, Opt o, double* __restrict__ keep, T* __restrict__ loss) {
    if (threadIdx.x != 0) return;
    double l = 0.0;
    for (int r = 0; r < p.R; ++r) {
        double* k = keep + KEEP_STRIDE * r;
        const double Nn = o.apply_mask ? k[4] : (double)p.rows * (double)p.r[r].F * (double)(p.r[r].nfft / 8);
        const bool fro = o.norm == 2;
        const double lin = fro ? sqrt(k[0]) : k[1], lg = fro ? sqrt(k[2]) : k[3];
        l += lin / Nn;
        k[KEEP_C0] = fro ? (k[0] > 0.0 ? 1.0 / (lin * Nn) : 0.0) : 1.0 / Nn;
        k[KEEP_C1] = 0.0;
        if (o.log_term) {
            l += o.alpha * lg / Nn;
            k[KEEP_C1] = fro ? (k[2] > 0.0 ? o.alpha / (lg * Nn) : 0.0) : o.alpha / Nn;
        }
        k[7] = 0.0;
    }
    keep[KEEP_LOSS] = l;
    loss[0] = (T)l;
}

// ---------------------------------------------------------------- backward: the gradient of a frame's windowed samples
template <typename T, int P>
__device__ inline void frame_grad(const T* __restrict__ yp, long sp, const T* __restrict__ yt, long st, long Tn, long f, const Res& q,
                                  const C* __restrict__ w, const cx<C>* __restrict__ tw, const Mel& mel, const Opt& o,
                                  const double* __restrict__ coef, cx<C>* A, cx<C>* Y, T* __restrict__ out, int tid) {
    constexpr int NC = Shape<P>::NC, NT = Shape<P>::NT, NM = Shape<P>::NM, NB = Shape<P>::NB;
    const double c0 = coef[KEEP_C0], c1 = coef[KEEP_C1];
    // one body for both signals (see the note at `both_signals`, criterion.h): the target, then the prediction, whose bins stay in Y.
    // The |X|^2 of a signal lie in A, free between the split and the next walk; dL/dm_p goes behind them.
    double mt[NB], mp[NB];
    double* Sp = reinterpret_cast<double*>(A);
    double* G = Sp + NC + 2;      // NM = NC / 4 doubles; A has 2 NC + 128
    both_signals<NB>(mt, mp, [&](int sig, double (&m)[NB]) {
        transform<T, P>(sig ? yp : yt, sig ? sp : st, Tn, f, q, w, tw, A, tid);
        for (int k = tid; k <= NC; k += NT) Y[k] = framed::split_bin<C, P, NTW>(A, tw, k);
        __syncthreads();
        for (int k = tid; k <= NC; k += NT) Sp[k] = power(Y[k]);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NB; ++i) m[i] = tid + NT * i < NM ? framed::mel_project<NC, NM>(Sp, mel, tid + NT * i) : 0.0;
        __syncthreads();
    });
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int j = tid + NT * i;
        if (j < NM) {
            const double mask = snr_mask(mt[i], o);
            const double d = (mt[i] - mp[i]) * mask;
            double g = c0 * (o.norm == 2 ? d : sign(d));
            if (o.log_term) {
                const double dl = (log(mt[i]) - log(mp[i])) * mask;
                g += c1 * (o.norm == 2 ? dl : sign(dl)) / mp[i];
            }
            G[j] = -mask * g;
        }
    }
    __syncthreads();
    const int* band = mel.idx + 3 * NM;
    const double* bw = mel.w + mel.nnz;
    // dL/dP[k] from the two bands of bin k; G = 2 dL/dP X, halved into the Hermitian spectrum of the inverse transform
    for (int k = tid; k <= NC; k += NT) {
        const int j = min(max(band[k], 0), NM - 2);
        const double dP = bw[2 * k] * G[j] + bw[2 * k + 1] * G[j + 1];
        Y[k] = framed::hermitian_half<C, P>(2.0 * dP, Y[k], k);
    }
    __syncthreads();
    if constexpr (Shape<P>::LONG) {
        framed::fft_wide<C, P, NTW, true>([&](int k) { return framed::unsplit<C, P, NTW>(Y, tw, k); }, A, tw, tid);
        framed::store_frame_grad_wide<T, C, P>(A, w, q, out, tid);
    } else {
        cx<C> v[P];
#pragma unroll
        for (int r = 0; r < P; ++r) v[r] = framed::unsplit<C, P, NTW>(Y, tw, tid + 64 * r);
        framed::fft_wave<C, P, NTW, true>(v, A, tw, tid);
        framed::store_frame_grad<T, C, P>(A, w, q, out, tid);
    }
}

template <typename T, bool LONG>
__global__ void __launch_bounds__(LONG ? NT_LONG : NT_SHORT)
melmss_frames_bwd_kernel(const T* __restrict__ yp, Strides sp, const T* __restrict__ yt, Strides st, Plan p, const C* __restrict__ wtab,
                         const cx<C>* __restrict__ tw, const int* __restrict__ melidx, const double* __restrict__ melw, Opt o,
                         const double* __restrict__ keep, T* __restrict__ gframes) {
    constexpr int NC_MAX = (LONG ? NFFT_MAX : NFFT_SHORT) / 2;
    __shared__ cx<C> A[NC_MAX + 64];
    __shared__ cx<C> Y[NC_MAX + 1];
    const int tid = threadIdx.x;
    int r;
    long row, f;
    locate<LONG>(p, blockIdx.x, r, row, f);
    const Res& q = p.r[r];
    const T* a = yp + row_offset(p, row, sp);
    const T* b = yt + row_offset(p, row, st);
    const C* w = wtab + q.w0;
    const Mel mel{melidx + q.mi0, melw + q.mw0, q.nnz};
    const double* coef = keep + KEEP_STRIDE * r;
    T* out = gframes + q.g0 + (row * q.F + f) * q.win;
    if constexpr (LONG) {
        if (q.nfft == 2048) frame_grad<T, 16>(a, sp.t, b, st.t, p.T, f, q, w, tw, mel, o, coef, A, Y, out, tid);
        else frame_grad<T, 32>(a, sp.t, b, st.t, p.T, f, q, w, tw, mel, o, coef, A, Y, out, tid);
    } else {
        switch (q.nfft) {
            case 128: frame_grad<T, 1>(a, sp.t, b, st.t, p.T, f, q, w, tw, mel, o, coef, A, Y, out, tid); break;
            case 256: frame_grad<T, 2>(a, sp.t, b, st.t, p.T, f, q, w, tw, mel, o, coef, A, Y, out, tid); break;
            case 512: frame_grad<T, 4>(a, sp.t, b, st.t, p.T, f, q, w, tw, mel, o, coef, A, Y, out, tid); break;
            default: frame_grad<T, 8>(a, sp.t, b, st.t, p.T, f, q, w, tw, mel, o, coef, A, Y, out, tid); break;
        }
    }
}

}  // namespace melmss
}  // namespace fl

using namespace fl;
using namespace fl::melmss;

extern "C" long fl_melmss_frames(long B, long T, long N, int R, int* res) {
    Plan p;
    return make_plan(B, T, N, R, res, p) ? p.frames : -1;
}
extern "C" long fl_melmss_gframe_elems(long B, long T, long N, int R, int* res) {
    Plan p;
    return make_plan(B, T, N, R, res, p) ? p.gelems : -1;
}
extern "C" long fl_melmss_keep_doubles(void) { return KEEP_DOUBLES; }
extern "C" long fl_melmss_mel_ints(int R, int* res) {
    Plan p;
    return make_tables(R, res, p) ? p.melints : -1;
}
extern "C" long fl_melmss_mel_doubles(int R, int* res) {
    Plan p;
    return make_tables(R, res, p) ? p.meldoubles : -1;
}
extern "C" long fl_melmss_launches(int R, int* res, int backward) {
    Plan p;
    if (!make_tables(R, res, p)) return -1;
    bool any[2] = {false, false};
    for (int r = 0; r < R; ++r) any[is_long(p.r[r].nfft)] = true;
    return (long)any[0] + (long)any[1] + (backward ? 1 : 2);
}

#define FL_MELMSS_PLAN(who)                                                                                                       \
    Plan p;                                                                                                                       \
    FL_REQUIRE(make_plan(B, Tn, N, R, res, p),                                                                                    \
               who ": bad sizes (1 <= R <= 8 resolutions (n_fft, hop, nnz), n_fft a power of two from 128 to 4096, hop >= 1, "    \
                   "n_fft / 2 < T <= 2^30, fewer than 2^31 frames and at most 2^38 samples in all, a mel table of 0 to "          \
                   "(n_fft / 8) (n_fft / 2 + 1) weights)");                                                                       \
    FL_REQUIRE(norm == 1 || norm == 2, who ": norm must be 1 or 2");                                                              \
    FL_REQUIRE(!apply_mask || noise_energy > 0.0, who ": apply_mask needs a noise_energy > 0");                                   \
    FL_REQUIRE((uintptr_t)tw % (2 * sizeof(C)) == 0, who ": the twiddle table must be aligned to its complex elements");          \
    const Opt o{norm, log_term ? 1 : 0, apply_mask ? 1 : 0, alpha_, threshold, noise_energy};                                     \
    const Strides sp{spb, spt, spc}, st{stb, stt, stc}

// (Tn: the header's T, the signals' length -- T is the precision here)
FL_ENTRY_F32_F64(fl_melmss_fwd, (const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long Tn,
                                 long N, int R, int* res, const void* wtab, const void* tw, const void* melidx, const void* melw,
                                 int norm, int log_term, double alpha, int apply_mask, double threshold, double noise_energy,
                                 void* partial, void* keep, void* loss, void* stream),
                 (yp, spb, spt, spc, yt, stb, stt, stc, B, Tn, N, R, res, wtab, tw, melidx, melw, norm, log_term, alpha, apply_mask,
                  threshold, noise_energy, partial, keep, loss, stream)) {
    FL_REQUIRE(yp && yt && res && wtab && tw && melidx && melw && partial && keep && loss, "melmss_fwd: null pointer");
    const double alpha_ = alpha;
    FL_MELMSS_PLAN("melmss_fwd");
    if (p.blocks[0] > 0) {
        hipLaunchKernelGGL((melmss_frames_kernel<T, false>), dim3((unsigned)p.blocks[0]), dim3(NT_SHORT), 0, (hipStream_t)stream,
                           (const T*)yp, sp, (const T*)yt, st, p, (const C*)wtab, (const cx<C>*)tw, (const int*)melidx,
                           (const double*)melw, o, (double*)partial);
        FL_CHECK_LAUNCH("melmss_frames (short)");
    }
    if (p.blocks[1] > 0) {
        hipLaunchKernelGGL((melmss_frames_kernel<T, true>), dim3((unsigned)p.blocks[1]), dim3(NT_LONG), 0, (hipStream_t)stream,
                           (const T*)yp, sp, (const T*)yt, st, p, (const C*)wtab, (const cx<C>*)tw, (const int*)melidx,
                           (const double*)melw, o, (double*)partial);
        FL_CHECK_LAUNCH("melmss_frames (long)");
    }
    const framed::Spans sums = framed::spans_of(p, [](const Res& q) { return q.fr0; }, [&](const Res& q) { return p.rows * q.F; });
    hipLaunchKernelGGL((framed::combine_kernel<NSUM, KEEP_STRIDE>), dim3((unsigned)p.R), dim3(256), 0, (hipStream_t)stream,
                       (const double*)partial, sums, (double*)keep);
    FL_CHECK_LAUNCH("melmss_combine");
    hipLaunchKernelGGL((melmss_final_kernel<T>), dim3(1), dim3(64), 0, (hipStream_t)stream, p, o, (double*)keep, (T*)loss);
    FL_CHECK_LAUNCH("melmss_final");
    return FL_OK;
}

FL_ENTRY_F32_F64(fl_melmss_bwd, (const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long Tn,
                                 long N, int R, int* res, const void* wtab, const void* tw, const void* melidx, const void* melw,
                                 int norm, int log_term, int apply_mask, double threshold, double noise_energy, const void* keep,
                                 const void* gloss, void* gframes, void* gy, void* stream),
                 (yp, spb, spt, spc, yt, stb, stt, stc, B, Tn, N, R, res, wtab, tw, melidx, melw, norm, log_term, apply_mask, threshold,
                  noise_energy, keep, gloss, gframes, gy, stream)) {
    FL_REQUIRE(yp && yt && res && wtab && tw && melidx && melw && keep && gloss && gframes && gy, "melmss_bwd: null pointer");
    const double alpha_ = 0.0;      // (folded into keep by the forward entry)
    FL_MELMSS_PLAN("melmss_bwd");
    if (p.blocks[0] > 0) {
        hipLaunchKernelGGL((melmss_frames_bwd_kernel<T, false>), dim3((unsigned)p.blocks[0]), dim3(NT_SHORT), 0, (hipStream_t)stream,
                           (const T*)yp, sp, (const T*)yt, st, p, (const C*)wtab, (const cx<C>*)tw, (const int*)melidx,
                           (const double*)melw, o, (const double*)keep, (T*)gframes);
        FL_CHECK_LAUNCH("melmss_frames_bwd (short)");
    }
    if (p.blocks[1] > 0) {
        hipLaunchKernelGGL((melmss_frames_bwd_kernel<T, true>), dim3((unsigned)p.blocks[1]), dim3(NT_LONG), 0, (hipStream_t)stream,
                           (const T*)yp, sp, (const T*)yt, st, p, (const C*)wtab, (const cx<C>*)tw, (const int*)melidx,
                           (const double*)melw, o, (const double*)keep, (T*)gframes);
        FL_CHECK_LAUNCH("melmss_frames_bwd (long)");
    }
    const long blocks = (p.rows * p.T + 255) / 256;
    hipLaunchKernelGGL((framed::ola_kernel<T, Plan>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const T*)gframes, p,
                       (const T*)gloss, (T*)gy);
    FL_CHECK_LAUNCH("melmss_ola");
    return FL_OK;
}
