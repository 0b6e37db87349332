// Energy decay curve criterion (gfx950 / MI355X): Schroeder's backward integral of a (B, T, N) signal, its level in dB, the
// squared error against a target's curve, and the gradient -- the reference's broadband `edc_loss`
// (flamo/optimize/loss.py:674-809), whose torch form is flip / square / cumsum / flip / divide / log10 twice, an MSE and the
// backward of all of it.
//
//   E[b,s,c] = sum_{s <= t < Tk} y[b,t,c]^2      e = 10 log10(E / Z)      Z = E[b,0,c] (energy_norm) or 1
//   loss = mean(m (e - e*)^2) [/ mean(e*~^2)]    m = 0 where the TARGET's curve is more than 60 dB under its start (clip)
//   dL/dy[b,t,c] = 2 y k (sum_{s <= t} w[s] - [energy_norm] sum_s w[s] E[s] / E[0]),   w = m (e - e*) / E
//
// One tiled scan serves the three passes.  Time is cut into tiles of TW = 64 * Q samples, one wavefront's share of one column:
// a lane owns Q consecutive samples, scans them in registers, and the lanes' totals are scanned with shuffles.  What a tile
// needs from the rest of its column is a sum of per-tile sums (a few hundred doubles at most), which a first launch leaves
// behind (edc_tsum_kernel) and the loss pass leaves behind for the backward pass -- so time is split over workgroups and a
// (1, 192000, 1) signal fills the device from one column.  A workgroup (4 wavefronts) stages a block of
// (seg tiles) x (NG <= 32 / sizeof(T) channels) through LDS with 16-byte accesses where the address allows, in either memory
// layout (include/flamo_hip_edc.h), so that no lane strides by N through HBM; its wavefronts then take the (tile, channel)
// units in turn and never talk to each other.  Every sum has a fixed order; tile sums, carries and partials are doubles.
#include "common.h"
#include "../../include/flamo_hip_edc.h"

namespace fl {
namespace edc {

constexpr int Q = 8;            // consecutive samples of one lane
constexpr int TW = 64 * Q;      // samples of a tile
constexpr int MAX_BLOCKS = 4096;   // partials fl_mean_square_final_* takes (reduce.hip)

template <typename T> struct Geo {
    static constexpr int NGMAX = 32 / (int)sizeof(T);     // channels of a group: 8 (float) / 4 (double)
    static constexpr int ELEMS = NGMAX * TW;              // samples of a staged block
    static constexpr int LDS = ELEMS + ELEMS / Q;         // ... with one pad per lane's run
    static constexpr int VEC = 16 / (int)sizeof(T);
};
template <typename T> struct alignas(16) V16 { T v[16 / sizeof(T)]; };

// the signal and how it is cut into blocks (host-made, passed by value)
struct Shape {
    int B, N, planar;
    long T, Tk, pitch;
    int nt;        // tiles of a column (over Tk)
    int G;         // channel groups
    int seg;       // tiles of a block
    int nts;       // blocks along time
    long nbt;      // blocks in all: B * G * nts
};

struct Block { int b, c0, NG, ts, TB; long t0; };

template <typename T>
__device__ inline Block block_of(const Shape& s, long bt) {
    Block k;
    k.ts = (int)(bt % s.nts);
    const long r = bt / s.nts;
    k.b = (int)(r / s.G);
    k.c0 = (int)(r % s.G) * Geo<T>::NGMAX;
    k.NG = min(Geo<T>::NGMAX, s.N - k.c0);
    k.TB = s.seg * TW;
    k.t0 = (long)k.ts * k.TB;
    return k;
}

// LDS place of sample t (from the block's start) of channel c (of the group).  A lane's run starts at a multiple of Q: with
// the pad its runs are an odd number of elements apart in either order, so the 32 lanes of an LDS access hit 32 banks.
template <bool PL>
__device__ inline int lidx(int t, int c, int NG, int TB) {
    if constexpr (PL) return c * (TB + TB / Q) + t + t / Q;
    return t * NG + c + t / Q;
}

// global memory -> LDS: the block's samples [t0, min(t0 + TB, tend)) of channels [c0, c0 + NG); the rest of the block is zero.
// PL: rows of `pitch` (time contiguous).  Otherwise (B, tlen, N) contiguous: a whole group (NG == N) is one contiguous range.
template <typename T, bool PL>
__device__ inline void load_block(T* lds, const T* base, const Shape& s, long tlen, const Block& k, long tend) {
    constexpr int VEC = Geo<T>::VEC;
    const int tid = threadIdx.x;
    const int nv = (int)max(0L, min((long)k.TB, tend - k.t0));
    if constexpr (PL) {
        for (int c = 0; c < k.NG; ++c) {
            const T* p = base + ((long)k.b * s.N + k.c0 + c) * s.pitch + k.t0;
            const int nvec = ((uintptr_t)p % 16 == 0) ? nv / VEC : 0;
            for (int i = tid; i < nvec; i += 256) {
                const V16<T> q = reinterpret_cast<const V16<T>*>(p)[i];
#pragma unroll
                for (int u = 0; u < VEC; ++u) lds[lidx<true>(i * VEC + u, c, k.NG, k.TB)] = q.v[u];
            }
            for (int t = nvec * VEC + tid; t < k.TB; t += 256) lds[lidx<true>(t, c, k.NG, k.TB)] = t < nv ? p[t] : (T)0;
        }
    } else {
        const T* p = base + ((long)k.b * tlen + k.t0) * s.N + k.c0;
        const int n = nv * k.NG, all = k.TB * k.NG;
        if (k.NG == s.N) {
            const int nvec = ((uintptr_t)p % 16 == 0) ? n / VEC : 0;
            for (int i = tid; i < nvec; i += 256) {
                const V16<T> q = reinterpret_cast<const V16<T>*>(p)[i];
#pragma unroll
                for (int u = 0; u < VEC; ++u) {
                    const int e = i * VEC + u, t = e / k.NG;
                    lds[lidx<false>(t, e - t * k.NG, k.NG, k.TB)] = q.v[u];
                }
            }
            for (int e = nvec * VEC + tid; e < all; e += 256) {
                const int t = e / k.NG;
                lds[lidx<false>(t, e - t * k.NG, k.NG, k.TB)] = e < n ? p[e] : (T)0;
            }
        } else {
            for (int e = tid; e < all; e += 256) {
                const int t = e / k.NG, c = e - t * k.NG;
                lds[lidx<false>(t, c, k.NG, k.TB)] = e < n ? p[(long)t * s.N + c] : (T)0;
            }
        }
    }
}

// LDS -> global memory, the same range; nothing outside it is written
template <typename T, bool PL>
__device__ inline void store_block(const T* lds, T* base, const Shape& s, long tlen, const Block& k, long tend) {
    constexpr int VEC = Geo<T>::VEC;
    const int tid = threadIdx.x;
    const int nv = (int)max(0L, min((long)k.TB, tend - k.t0));
    if constexpr (PL) {
        for (int c = 0; c < k.NG; ++c) {
            T* p = base + ((long)k.b * s.N + k.c0 + c) * s.pitch + k.t0;
            const int nvec = ((uintptr_t)p % 16 == 0) ? nv / VEC : 0;
            for (int i = tid; i < nvec; i += 256) {
                V16<T> q;
#pragma unroll
                for (int u = 0; u < VEC; ++u) q.v[u] = lds[lidx<true>(i * VEC + u, c, k.NG, k.TB)];
                reinterpret_cast<V16<T>*>(p)[i] = q;
            }
            for (int t = nvec * VEC + tid; t < nv; t += 256) p[t] = lds[lidx<true>(t, c, k.NG, k.TB)];
        }
    } else {
        T* p = base + ((long)k.b * tlen + k.t0) * s.N + k.c0;
        const int n = nv * k.NG;
        if (k.NG == s.N) {
            const int nvec = ((uintptr_t)p % 16 == 0) ? n / VEC : 0;
            for (int i = tid; i < nvec; i += 256) {
                V16<T> q;
#pragma unroll
                for (int u = 0; u < VEC; ++u) {
                    const int e = i * VEC + u, t = e / k.NG;
                    q.v[u] = lds[lidx<false>(t, e - t * k.NG, k.NG, k.TB)];
                }
                reinterpret_cast<V16<T>*>(p)[i] = q;
            }
            for (int e = nvec * VEC + tid; e < n; e += 256) {
                const int t = e / k.NG;
                p[e] = lds[lidx<false>(t, e - t * k.NG, k.NG, k.TB)];
            }
        } else {
            for (int e = tid; e < n; e += 256) {
                const int t = e / k.NG, c = e - t * k.NG;
                p[(long)t * s.N + c] = lds[lidx<false>(t, c, k.NG, k.TB)];
            }
        }
    }
}

// sum of a[lo .. hi) over the wavefront, the same order whoever asks
__device__ inline double wave_sum_range(const double* __restrict__ a, int lo, int hi, int lane) {
    double s = 0.0;
    for (int j = lo + lane; j < hi; j += 64) s += a[j];
    return wave_sum(s);
}
// sum of `tot` over the lanes above this one / below this one
__device__ inline double wave_above(double tot, int lane) {
    double inc = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_down(inc, off, 64);
        if (lane + off < 64) inc += o;
    }
    const double ex = __shfl_down(inc, 1, 64);
    return lane == 63 ? 0.0 : ex;
}
__device__ inline double wave_below(double tot, int lane) {
    double inc = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    const double ex = __shfl_up(inc, 1, 64);
    return lane == 0 ? 0.0 : ex;
}

// 10 log10(E / Z) in the signal's precision, the reference's order of operations (divide, log10, times ten)
template <typename T> __device__ inline T level_db(double E, double Z) { return (T)10 * log10((T)(E / Z)); }

// the block's partial of a loss sum: wavefronts in a fixed order
__device__ inline void block_partial(double acc, double* red, double* partial) {
    acc = wave_sum(acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------- sum of y^2 per (column, tile)
template <typename T, bool PL>
__global__ void __launch_bounds__(256) edc_tsum_kernel(const T* __restrict__ y, Shape s, double* __restrict__ tsum) {
    __shared__ T A[Geo<T>::LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long bt = blockIdx.x; bt < s.nbt; bt += gridDim.x) {
        const Block k = block_of<T>(s, bt);
        load_block<T, PL>(A, y, s, s.T, k, s.Tk);
        __syncthreads();
        for (int u = wave; u < k.NG * s.seg; u += 4) {
            const int c = u % k.NG, sg = u / k.NG, j = k.ts * s.seg + sg;
            if (j >= s.nt) continue;
            const int tl = sg * TW + lane * Q;
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const double v = (double)A[lidx<PL>(tl + q, c, k.NG, k.TB)];
                a += v * v;
            }
            a = wave_sum(a);
            if (lane == 0) tsum[((long)k.b * s.N + k.c0 + c) * s.nt + j] = a;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- the curve in dB (and the target's mean square)
template <typename T, bool PL>
__global__ void __launch_bounds__(256) edc_curve_kernel(const T* __restrict__ y, Shape s, const double* __restrict__ tsum,
                                                       int energy_norm, int clip, T* __restrict__ edb,
                                                       double* __restrict__ partial) {
    __shared__ T A[Geo<T>::LDS];
    __shared__ T O[Geo<T>::LDS];
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    for (long bt = blockIdx.x; bt < s.nbt; bt += gridDim.x) {
        const Block k = block_of<T>(s, bt);
        load_block<T, PL>(A, y, s, s.T, k, s.Tk);
        __syncthreads();
        for (int u = wave; u < k.NG * s.seg; u += 4) {
            const int c = u % k.NG, sg = u / k.NG, j = k.ts * s.seg + sg;
            if (j >= s.nt) continue;
            const double* col = tsum + ((long)k.b * s.N + k.c0 + c) * s.nt;
            const double carry = wave_sum_range(col, j + 1, s.nt, lane);
            const double E0 = (energy_norm || clip) ? wave_sum_range(col, 0, s.nt, lane) : 1.0;
            const double Z = energy_norm ? E0 : 1.0;
            const T thr = level_db<T>(E0, Z) - (T)60;
            const int tl = sg * TW + lane * Q;
            double sfx[Q];
            double run = 0.0;
#pragma unroll
            for (int q = Q - 1; q >= 0; --q) {
                const double v = (double)A[lidx<PL>(tl + q, c, k.NG, k.TB)];
                run += v * v;
                sfx[q] = run;
            }
            const double above = carry + wave_above(run, lane);
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const T e = level_db<T>(above + sfx[q], Z);
                O[lidx<false>(tl + q, c, k.NG, k.TB)] = e;
                if (partial != nullptr && k.t0 + tl + q < s.Tk) {
                    const double ec = (clip && e < thr) ? -180.0 : (double)e;
                    acc += ec * ec;
                }
            }
        }
        __syncthreads();
        store_block<T, false>(O, edb, s, s.Tk, k, s.Tk);
        __syncthreads();
    }
    if (partial != nullptr) block_partial(acc, red, partial);
}

// ---------------------------------------------------------------- squared error of the curves; w and its tile sums
template <typename T, bool PL>
__global__ void __launch_bounds__(256) edc_loss_kernel(const T* __restrict__ y, Shape s, const double* __restrict__ tsum,
                                                      const T* __restrict__ edb_true, const double* __restrict__ tsum_true,
                                                      int energy_norm, int clip, T* __restrict__ w, double* __restrict__ wsum,
                                                      double* __restrict__ wesum, double* __restrict__ partial) {
    __shared__ T A[Geo<T>::LDS];
    __shared__ T R[Geo<T>::LDS];
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    for (long bt = blockIdx.x; bt < s.nbt; bt += gridDim.x) {
        const Block k = block_of<T>(s, bt);
        load_block<T, PL>(A, y, s, s.T, k, s.Tk);
        load_block<T, false>(R, edb_true, s, s.Tk, k, s.Tk);
        __syncthreads();
        for (int u = wave; u < k.NG * s.seg; u += 4) {
            const int c = u % k.NG, sg = u / k.NG, j = k.ts * s.seg + sg;
            if (j >= s.nt) continue;
            const long cj = ((long)k.b * s.N + k.c0 + c) * s.nt;
            const double carry = wave_sum_range(tsum + cj, j + 1, s.nt, lane);
            const double Z = energy_norm ? wave_sum_range(tsum + cj, 0, s.nt, lane) : 1.0;
            T thr = (T)0;
            if (clip) {      // the target's own start level, formed as edc_curve_kernel formed it
                const double E0t = wave_sum_range(tsum_true + cj, 0, s.nt, lane);
                thr = level_db<T>(E0t, energy_norm ? E0t : 1.0) - (T)60;
            }
            const int tl = sg * TW + lane * Q;
            double sfx[Q];
            double run = 0.0;
#pragma unroll
            for (int q = Q - 1; q >= 0; --q) {
                const double v = (double)A[lidx<PL>(tl + q, c, k.NG, k.TB)];
                run += v * v;
                sfx[q] = run;
            }
            const double above = carry + wave_above(run, lane);
            double sw = 0.0, swe = 0.0;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const double E = above + sfx[q];
                const T es = R[lidx<false>(tl + q, c, k.NG, k.TB)];
                const bool m = (k.t0 + tl + q < s.Tk) && !(clip && es < thr);
                T wq = (T)0;
                if (m) {
                    const T d = level_db<T>(E, Z) - es;
                    acc += (double)d * (double)d;
                    wq = (T)((double)d / E);
                    sw += (double)wq;
                    swe += (double)d;
                }
                A[lidx<PL>(tl + q, c, k.NG, k.TB)] = wq;
            }
            sw = wave_sum(sw);
            swe = wave_sum(swe);
            if (lane == 0) {
                wsum[cj + j] = sw;
                wesum[cj + j] = swe;
            }
        }
        __syncthreads();
        if (w != nullptr) store_block<T, PL>(A, w, s, s.T, k, s.Tk);
        __syncthreads();
    }
    block_partial(acc, red, partial);
}

template <typename T>
__global__ void edc_ratio_kernel(T* __restrict__ loss, const T* __restrict__ den) { loss[0] = loss[0] / den[0]; }

// ---------------------------------------------------------------- gradient: a forward scan of w
template <typename T, bool PL>
__global__ void __launch_bounds__(256) edc_bwd_kernel(const T* __restrict__ y, Shape s, const double* __restrict__ tsum,
                                                     const T* __restrict__ w, const double* __restrict__ wsum,
                                                     const double* __restrict__ wesum, const T* __restrict__ gloss,
                                                     const T* __restrict__ den, int energy_norm, double coef, T* __restrict__ gy) {
    __shared__ T A[Geo<T>::LDS];
    __shared__ T W[Geo<T>::LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double kk = 2.0 * coef * (double)gloss[0] / (den != nullptr ? (double)den[0] : 1.0);
    for (long bt = blockIdx.x; bt < s.nbt; bt += gridDim.x) {
        const Block k = block_of<T>(s, bt);
        load_block<T, PL>(A, y, s, s.T, k, s.Tk);
        load_block<T, PL>(W, w, s, s.T, k, s.Tk);
        __syncthreads();
        for (int u = wave; u < k.NG * s.seg; u += 4) {
            const int c = u % k.NG, sg = u / k.NG, j = k.ts * s.seg + sg;
            const int tl = sg * TW + lane * Q;
            if (j >= s.nt) continue;      // past Tk: the block was loaded as zeros, and zeros are what goes out
            const long cj = ((long)k.b * s.N + k.c0 + c) * s.nt;
            const double before = wave_sum_range(wsum + cj, 0, j, lane);
            double sub = 0.0;
            if (energy_norm) sub = wave_sum_range(wesum + cj, 0, s.nt, lane) / wave_sum_range(tsum + cj, 0, s.nt, lane);
            double pfx[Q];
            double run = 0.0;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                run += (double)W[lidx<PL>(tl + q, c, k.NG, k.TB)];
                pfx[q] = run;
            }
            const double below = before + wave_below(run, lane);
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int at = lidx<PL>(tl + q, c, k.NG, k.TB);
                // exactly zero from Tk on, whatever the sums hold (a column with a silent tail has infinite ones)
                A[at] = k.t0 + tl + q < s.Tk ? (T)(kk * (double)A[at] * ((below + pfx[q]) - sub)) : (T)0;
            }
        }
        __syncthreads();
        store_block<T, PL>(A, gy, s, s.T, k, s.T);
        __syncthreads();
    }
}

// blocks along time cover `tcover` samples (Tk forward, T backward: the gradient's zeros from Tk on are written too)
template <typename T>
static Shape make_shape(int planar, int B, long Tlen, long Tk, int N, long pitch, long tcover) {
    Shape s;
    s.B = B; s.N = N; s.planar = planar; s.T = Tlen; s.Tk = Tk; s.pitch = pitch;
    s.nt = cdiv_i(Tk, TW);
    s.G = cdiv_i(N, Geo<T>::NGMAX);
    const int ng = N < Geo<T>::NGMAX ? N : Geo<T>::NGMAX;
    s.seg = Geo<T>::NGMAX / ng;
    s.nts = cdiv_i(cdiv_i(tcover, TW), s.seg);
    s.nbt = (long)B * s.G * s.nts;
    return s;
}
// at most MAX_BLOCKS workgroups (one loss partial each), every one with the same number of blocks but the last
static unsigned grid_of(const Shape& s) {
    const long rounds = (s.nbt + MAX_BLOCKS - 1) / MAX_BLOCKS;
    return (unsigned)((s.nbt + rounds - 1) / rounds);
}

#define FL_EDC_SIZES(who)                                                                                          \
    FL_REQUIRE(B > 0 && N > 0 && Tk > 0 && Tn >= Tk, who ": bad sizes (B, N > 0, 0 < Tk <= T)");                    \
    FL_REQUIRE(!planar || pitch >= Tn, who ": planar rows need pitch >= T");                                       \
    FL_REQUIRE((Tn + TW - 1) / TW < (1L << 24) && (long)B * N < (1L << 31), who ": signal too large")

template <typename T>
static int final_of(const void* parts, int n, double inv, void* out, void* stream) {
    if constexpr (std::is_same<T, float>::value) return fl_mean_square_final_f32(parts, n, inv, out, stream);
    else return fl_mean_square_final_f64(parts, n, inv, out, stream);
}

}  // namespace edc
}  // namespace fl

using namespace fl;
using namespace fl::edc;

extern "C" int fl_edc_tile(void) { return TW; }

#define FL_EDC_LAUNCH(KERNEL, ...)                                                                                 \
    do {                                                                                                           \
        if (planar) hipLaunchKernelGGL((KERNEL<T, true>), dim3(grid_of(s)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);   \
        else hipLaunchKernelGGL((KERNEL<T, false>), dim3(grid_of(s)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);         \
    } while (0)

// (Tn: the header's T, the signal's length -- T is the precision here)
FL_ENTRY_F32_F64(fl_edc_tile_sums, (const void* y, int planar, int B, long Tn, long Tk, int N, long pitch, void* tsum, void* stream),
                 (y, planar, B, Tn, Tk, N, pitch, tsum, stream)) {
    FL_REQUIRE(y && tsum, "edc_tile_sums: null pointer");
    FL_EDC_SIZES("edc_tile_sums");
    const Shape s = make_shape<T>(planar, B, Tn, Tk, N, pitch, Tk);
    FL_EDC_LAUNCH(edc_tsum_kernel, (const T*)y, s, (double*)tsum);
    FL_CHECK_LAUNCH("edc_tile_sums");
    return FL_OK;
}

FL_ENTRY_F32_F64(fl_edc_curve, (const void* y, int planar, int B, long Tn, long Tk, int N, long pitch, const void* tsum, int energy_norm,
                                int clip, void* edb, void* den, void* scratch, void* stream),
                 (y, planar, B, Tn, Tk, N, pitch, tsum, energy_norm, clip, edb, den, scratch, stream)) {
    FL_REQUIRE(y && tsum && edb, "edc_curve: null pointer");
    FL_REQUIRE(!den || scratch, "edc_curve: the target's mean square needs the scratch buffer");
    FL_EDC_SIZES("edc_curve");
    const Shape s = make_shape<T>(planar, B, Tn, Tk, N, pitch, Tk);
    FL_EDC_LAUNCH(edc_curve_kernel, (const T*)y, s, (const double*)tsum, energy_norm, clip, (T*)edb, den ? (double*)scratch : nullptr);
    FL_CHECK_LAUNCH("edc_curve");
    if (den) return final_of<T>(scratch, (int)grid_of(s), 1.0 / ((double)B * (double)Tk * (double)N), den, stream);
    return FL_OK;
}

FL_ENTRY_F32_F64(fl_edc_loss, (const void* y, int planar, int B, long Tn, long Tk, int N, long pitch, const void* tsum, const void* edb_true,
                               const void* tsum_true, int energy_norm, int clip, const void* den, void* w, void* wsum, void* wesum,
                               void* loss, void* scratch, void* stream),
                 (y, planar, B, Tn, Tk, N, pitch, tsum, edb_true, tsum_true, energy_norm, clip, den, w, wsum, wesum, loss, scratch, stream)) {
    FL_REQUIRE(y && tsum && edb_true && tsum_true && wsum && wesum && loss && scratch, "edc_loss: null pointer");
    FL_EDC_SIZES("edc_loss");
    const Shape s = make_shape<T>(planar, B, Tn, Tk, N, pitch, Tk);
    FL_EDC_LAUNCH(edc_loss_kernel, (const T*)y, s, (const double*)tsum, (const T*)edb_true, (const double*)tsum_true, energy_norm, clip,
                  (T*)w, (double*)wsum, (double*)wesum, (double*)scratch);
    FL_CHECK_LAUNCH("edc_loss");
    const int rc = final_of<T>(scratch, (int)grid_of(s), 1.0 / ((double)B * (double)Tk * (double)N), loss, stream);
    if (rc != FL_OK || !den) return rc;
    hipLaunchKernelGGL((edc_ratio_kernel<T>), dim3(1), dim3(1), 0, (hipStream_t)stream, (T*)loss, (const T*)den);
    FL_CHECK_LAUNCH("edc_ratio");
    return FL_OK;
}

FL_ENTRY_F32_F64(fl_edc_bwd, (const void* y, int planar, int B, long Tn, long Tk, int N, long pitch, const void* tsum, const void* w,
                              const void* wsum, const void* wesum, const void* gloss, const void* den, int energy_norm, void* gy,
                              void* stream),
                 (y, planar, B, Tn, Tk, N, pitch, tsum, w, wsum, wesum, gloss, den, energy_norm, gy, stream)) {
    FL_REQUIRE(y && tsum && w && wsum && wesum && gloss && gy, "edc_bwd: null pointer");
    FL_EDC_SIZES("edc_bwd");
    const Shape s = make_shape<T>(planar, B, Tn, Tk, N, pitch, Tn);
    const double coef = 2.0 / ((double)B * (double)Tk * (double)N) * (10.0 / 2.302585092994045684);
    FL_EDC_LAUNCH(edc_bwd_kernel, (const T*)y, s, (const double*)tsum, (const T*)w, (const double*)wsum, (const double*)wesum,
                  (const T*)gloss, (const T*)den, energy_norm, coef, (T*)gy);
    FL_CHECK_LAUNCH("edc_bwd");
    return FL_OK;
}
