// The framed real transform of the short-time criteria (avgpow.hip, mrstft.hip, edr.hip), one wavefront per frame: the
// wave-level pieces only -- the kernels, their plans and LDS arrays are the callers'.  (What the criteria on (B, T, N) signals
// share around it -- rows, the mel projection, the combine, the multi-resolution overlap-add -- is criterion.h.)
//
// The n_fft = 128 P real samples of a frame are Nc = 64 P complex ones (even samples real, odd samples imaginary), P = 2, 4, 8,
// 16 per lane.  The window is applied while loading and only the samples under its support [lpad, lpad + win) are read.  The
// packed transform is a Stockham walk of three passes, radix P x 8 x 8, every pass an in-register transform of regfft.h: the
// first straight on the loaded values (lane j holds z[j + 64 r]), the two radix-8 passes on 8 P butterflies (P / 8 per lane;
// with P < 8 the lanes from 8 P on idle), with an exchange through LDS behind each.  The Nc + 1 bins of the real transform are
// split from the packed one bin by bin; the way back is the adjoint of the split (unsplit), the inverse walk and the windowed
// store, and an overlap-add that gathers per sample with the reflected margins folded back onto the samples they mirror.
//
// n_fft = 128 (P = 1, for melmss.hip) is the same walk with an empty first pass: 1 x 8 x 8, eight lanes busy in each radix-8
// pass, A[128] with every value at twice its index.
//
// n_fft = 4096 (P = 32) does not fit one wavefront: 32 complex doubles per lane are 128 VGPRs before a radix-32's temporaries,
// beside the 200 the P = 16 backward kernel already needs.  The WIDE walk below gives a frame to a workgroup of WIDE_NT = 256
// threads (four wavefronts) instead: four passes, radix (P / 8) x 8 x 8 x 8, the first on values as they are loaded (two
// butterflies per thread, never more than four values held), then 8 P radix-8 butterflies per pass, one per thread, with an
// LDS exchange behind each -- one exchange more than the three-pass walk, the 8 values of one butterfly per thread, no scratch.
// It also takes P = 16 (2 x 8 x 8 x 8, half the threads busy in the radix-8 passes), so that a caller can run 2048 and 4096
// in one launch of one workgroup size.  split_bin, unsplit and hermitian_half serve both walks.
//
// Template parameters: T the signals' type, C the transform's (window, twiddles and LDS have it), NTW the length of the
// caller's twiddle table, tw[j] = exp(-2 pi i j / NTW), a multiple of n_fft.
//
// LDS.  A[64 P + 64] complex values, index i stored at i + (i >> log2 P): one pad per P values, so that the first pass's
// stores (lane j writes j P + t: with doubles a stride of P + 1 values = 4 (P + 1) dwords, whose gcd with the 64 banks is 4 =
// the width of one value) and the radix-8 passes' loads (consecutive j) both spread over all banks.
//
// Registers, 16 doubles per lane (n_fft = 2048): the 16 complex doubles of a pass are 64 VGPRs; a radix-16 transform of
// regfft.h holds its input, the intermediate products and four-value temporaries at once -- mrstft.hip's kernels come to 170
// and 200 VGPRs with no scratch, under the 256 of two wavefronts per SIMD.
//
// Inlining is left to the compiler, and a caller with one frame shape may ask for it at the call ([[clang::always_inline]], as
// avgpow.hip does: the compiler makes frame_transform a function of its own there).  An always-inline attribute here is
// not the same thing: it inlines the walk before it is simplified, and in mrstft.hip's n_fft = 2048 inverse pass the backend
// then fuses the other product of a twiddle multiplication into its FMA -- the float64 gradient moves in its last bit.
#pragma once
#include "common.h"
#include "regfft.h"

namespace fl {
namespace framed {

// where a frame sits: frame f starts at padded sample f * hop, its window covers [lpad, lpad + win) of the n_fft samples
struct Frame {
    int hop, win, lpad;
};

template <int P> struct Log2;
template <> struct Log2<1> { static constexpr int v = 0; };
template <> struct Log2<32> { static constexpr int v = 5; };
template <> struct Log2<2> { static constexpr int v = 1; };
template <> struct Log2<4> { static constexpr int v = 2; };
template <> struct Log2<8> { static constexpr int v = 3; };
template <> struct Log2<16> { static constexpr int v = 4; };

template <int P>
__device__ inline int zp(int i) { return i + (i >> Log2<P>::v); }

// One radix-8 Stockham pass over the 64 P values in A, NS = the product of the radices before it: butterfly j reads
// A[j + t 8 P], t < 8, multiplies by W_{8 NS}^(t (j mod NS)) and writes A[(j / NS) 8 NS + (j mod NS) + t NS].
template <typename C, int P, int NTW, int NS, bool INV>
__device__ inline void pass8(cx<C>* A, const cx<C>* __restrict__ tw, int lane) {
    constexpr int NBF = 8 * P, NI = P >= 8 ? P / 8 : 1, STEP = NTW / (8 * NS);
    cx<C> u[NI][8];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = lane + 64 * i;
        if (j < NBF) {
            const int jm = j & (NS - 1);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                u[i][t] = A[zp<P>(j + t * NBF)];
                if (t > 0) {
                    const cx<C> w = tw[t * jm * STEP];
                    u[i][t] = mul_plain(u[i][t], INV ? conj(w) : w);
                }
            }
            RegFFT<C, 8, INV>::run(u[i]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = lane + 64 * i;
        if (j < NBF) {
            const int jm = j & (NS - 1), base = (j - jm) * 8 + jm;
#pragma unroll
            for (int t = 0; t < 8; ++t) A[zp<P>(base + t * NS)] = u[i][t];
        }
    }
    __syncthreads();
}

// Z[k] = sum_n z[n] exp(-+2 pi i k n / (64 P)) by one wavefront.  In: v[r] = z[lane + 64 r].  Out: A[zp(k)] = Z[k], visible
// to every lane.
template <typename C, int P, int NTW, bool INV>
__device__ inline void fft_wave(cx<C> (&v)[P], cx<C>* A, const cx<C>* __restrict__ tw, int lane) {
    static_assert(NTW % (128 * P) == 0, "the twiddle table must hold the n_fft-th roots");
    RegFFT<C, P, INV>::run(v);
#pragma unroll
    for (int t = 0; t < P; ++t) A[zp<P>(lane * P + t)] = v[t];
    __syncthreads();
    pass8<C, P, NTW, P, INV>(A, tw, lane);
    pass8<C, P, NTW, 8 * P, INV>(A, tw, lane);
}

// sample j of the row reflect-padded by `half` on each side (j counted from the first padded sample); T > half
template <typename T>
__device__ inline T padded(const T* __restrict__ y, long stride, long Tn, long j, int half) {
    long t = j - half;
    if (t < 0) t = -t;
    if (t >= Tn) t = 2 * (Tn - 1) - t;
    return y[t * stride];
}

// the windowed frame f as 64 P complex values (even samples real, odd samples imaginary), transformed into A; only the
// samples under the window are read
template <typename T, typename C, int P, int NTW>
__device__ inline void frame_transform(const T* __restrict__ y, long stride, long Tn, long f, const Frame& q, const C* __restrict__ w,
                                       const cx<C>* __restrict__ tw, cx<C>* A, int lane) {
    cx<C> v[P];
    const long j0 = f * q.hop;
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const int n = 2 * (lane + 64 * r) - q.lpad;      // place under the window of the even sample
        C re = 0, im = 0;
        if (n >= 0 && n < q.win) re = (C)padded(y, stride, Tn, j0 + n + q.lpad, 64 * P) * w[n];
        if (n + 1 >= 0 && n + 1 < q.win) im = (C)padded(y, stride, Tn, j0 + n + 1 + q.lpad, 64 * P) * w[n + 1];
        v[r] = cx<C>(re, im);
    }
    fft_wave<C, P, NTW, false>(v, A, tw, lane);
}

// bin k (0 .. Nc) of the real transform from the packed one: X[k] = E[k] + W_{2 Nc}^k O[k],
// E = (Z[k] + conj Z[Nc - k]) / 2, O = -i (Z[k] - conj Z[Nc - k]) / 2
template <typename C, int P, int NTW>
__device__ inline cx<C> split_bin(const cx<C>* A, const cx<C>* __restrict__ tw, int k) {
    constexpr int NC = 64 * P;
    if (k == NC) {
        const cx<C> z = A[0];
        return cx<C>(z.x - z.y, (C)0);
    }
    const cx<C> a = A[zp<P>(k)], b = conj(A[zp<P>((NC - k) & (NC - 1))]);
    const cx<C> e = (C)0.5 * (a + b), o = (C)0.5 * mul_mi(a - b);
    return e + mul_plain(o, tw[k * (NTW / (2 * NC))]);
}

// Bin k of the Hermitian spectrum whose inverse transform is Re sum_{k <= Nc} G[k] exp(+2 pi i k n / n_fft), G = s x:
// G / 2 inside, Re G at the two ends
template <typename C, int P>
__device__ inline cx<C> hermitian_half(C s, cx<C> x, int k) {
    return (k == 0 || k == 64 * P) ? cx<C>(s * x.x, (C)0) : cx<C>((C)0.5 * s * x.x, (C)0.5 * s * x.y);
}

// The adjoint of the split, as the input of the inverse walk: with Y[0 .. Nc] of hermitian_half, a lane's v[r] at k = lane + 64 r,
// v[m] = y[2 m] + i y[2 m + 1] = sum_{k < Nc} ((Y[k] + conj Y[Nc - k]) + i conj(W^k) (Y[k] - conj Y[Nc - k])) exp(+2 pi i k m / Nc)
template <typename C, int P, int NTW>
__device__ inline cx<C> unsplit(const cx<C>* Y, const cx<C>* __restrict__ tw, int k) {
    constexpr int NC = 64 * P;
    const cx<C> a = Y[k], b = conj(Y[NC - k]);
    return (a + b) + mul_i(mul_plain(a - b, conj(tw[k * (NTW / (2 * NC))])));
}

// the win samples of the frame's gradient under the window, from the inverse walk's A: out[n] = y[n + lpad] w[n]
template <typename T, typename C, int P>
__device__ inline void store_frame_grad(const cx<C>* A, const C* __restrict__ w, const Frame& q, T* __restrict__ out, int lane) {
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const int m = lane + 64 * r, n = 2 * m - q.lpad;
        const cx<C> z = A[zp<P>(m)];
        if (n >= 0 && n < q.win) out[n] = (T)(z.x * w[n]);
        if (n + 1 >= 0 && n + 1 < q.win) out[n + 1] = (T)(z.y * w[n + 1]);
    }
}

// Overlap-add as a gather, in a fixed order: adds to acc the gradients that the frames 0 .. last of a row (frame f's win
// values at g + f win) hold for sample t of its Tn samples -- the frames that cover the sample itself, then those that cover
// its image in the left reflected margin, then in the right one, first frame to last inside each.  True when there was one.
template <typename T>
__device__ inline bool gather_sample(const T* __restrict__ g, long t, long Tn, int half, const Frame& q, long last, double& acc) {
    bool any = false;
    // the frames that hold the padded sample j under their window, first to last
    auto gather = [&](long j) {
        const long hi = j - q.lpad, lo = hi - q.win + 1;
        if (hi < 0) return;
        const long f0 = lo <= 0 ? 0 : (lo + q.hop - 1) / q.hop;
        const long f1 = min(last, hi / q.hop);
        for (long f = f0; f <= f1; ++f) {
            acc += (double)g[f * q.win + (hi - f * q.hop)];
            any = true;
        }
    };
    gather(t + half);                                          // the sample itself
    if (t >= 1 && t <= half) gather(half - t);                 // its image in the left margin
    if (t <= Tn - 2) gather(2 * (Tn - 1) - t + half);          // ... in the right margin (frames beyond the last hold none)
    return any;
}

// ---------------------------------------------------------------- the wide walk: one frame per workgroup of WIDE_NT threads
constexpr int WIDE_NT = 256;

// One radix-8 Stockham pass over the 64 P values in A, one butterfly per thread (8 P <= WIDE_NT of them); indices as in pass8.
template <typename C, int P, int NTW, int NS, bool INV>
__device__ inline void pass8_wide(cx<C>* A, const cx<C>* __restrict__ tw, int tid) {
    constexpr int NBF = 8 * P, STEP = NTW / (8 * NS);
    static_assert(NBF <= WIDE_NT, "one butterfly per thread");
    cx<C> u[8];
    const int jm = tid & (NS - 1);
    if (tid < NBF) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            u[t] = A[zp<P>(tid + t * NBF)];
            if (t > 0) {
                const cx<C> w = tw[t * jm * STEP];
                u[t] = mul_plain(u[t], INV ? conj(w) : w);
            }
        }
        RegFFT<C, 8, INV>::run(u);
    }
    __syncthreads();
    if (tid < NBF) {
        const int base = (tid - jm) * 8 + jm;
#pragma unroll
        for (int t = 0; t < 8; ++t) A[zp<P>(base + t * NS)] = u[t];
    }
    __syncthreads();
}

// Z[k] = sum_n z[n] exp(-+2 pi i k n / (64 P)) by WIDE_NT threads, P = 16 or 32.  In: z(n), a callable every thread may ask
// for any n < 64 P (it must not read A).  Out: A[zp(k)] = Z[k], visible to every thread.  The caller has a barrier between
// its last read of A and this call.
template <typename C, int P, int NTW, bool INV, class Z>
__device__ inline void fft_wide(Z&& z, cx<C>* A, const cx<C>* __restrict__ tw, int tid) {
    static_assert(P == 16 || P == 32, "the wide walk is (P / 8) x 8 x 8 x 8");
    static_assert(NTW % (128 * P) == 0, "the twiddle table must hold the n_fft-th roots");
    constexpr int R0 = P / 8, NB0 = 64 * P / R0;      // 512 first-pass butterflies: z[j + 512 t], t < R0, to A[j R0 + t]
    for (int j = tid; j < NB0; j += WIDE_NT) {
        cx<C> v[R0];
#pragma unroll
        for (int t = 0; t < R0; ++t) v[t] = z(j + t * NB0);
        RegFFT<C, R0, INV>::run(v);
#pragma unroll
        for (int t = 0; t < R0; ++t) A[zp<P>(j * R0 + t)] = v[t];
    }
    __syncthreads();
    pass8_wide<C, P, NTW, R0, INV>(A, tw, tid);
    pass8_wide<C, P, NTW, 8 * R0, INV>(A, tw, tid);
    pass8_wide<C, P, NTW, 64 * R0, INV>(A, tw, tid);
}

// frame_transform by WIDE_NT threads
template <typename T, typename C, int P, int NTW>
__device__ inline void frame_transform_wide(const T* __restrict__ y, long stride, long Tn, long f, const Frame& q, const C* __restrict__ w,
                                            const cx<C>* __restrict__ tw, cx<C>* A, int tid) {
    const long j0 = f * q.hop;
    fft_wide<C, P, NTW, false>(
        [&](int m) {
            const int n = 2 * m - q.lpad;      // place under the window of the even sample
            C re = 0, im = 0;
            if (n >= 0 && n < q.win) re = (C)padded(y, stride, Tn, j0 + n + q.lpad, 64 * P) * w[n];
            if (n + 1 >= 0 && n + 1 < q.win) im = (C)padded(y, stride, Tn, j0 + n + 1 + q.lpad, 64 * P) * w[n + 1];
            return cx<C>(re, im);
        },
        A, tw, tid);
}

// store_frame_grad by WIDE_NT threads
template <typename T, typename C, int P>
__device__ inline void store_frame_grad_wide(const cx<C>* A, const C* __restrict__ w, const Frame& q, T* __restrict__ out, int tid) {
    for (int m = tid; m < 64 * P; m += WIDE_NT) {
        const int n = 2 * m - q.lpad;
        const cx<C> z = A[zp<P>(m)];
        if (n >= 0 && n < q.win) out[n] = (T)(z.x * w[n]);
        if (n + 1 >= 0 && n + 1 < q.win) out[n + 1] = (T)(z.y * w[n + 1]);
    }
}

}  // namespace framed
}  // namespace fl
