// What the criteria on (B, T, N) signals share around the framed transform of framed.h (mrstft.hip, edr.hip, melmss.hip,
// mss.hip): how a row of the signals is found, the mel table and its projection, the mask and the sign of the multi-scale
// criteria, the one loop body for both signals, the combine of the frames' partial sums, the multi-resolution overlap-add and
// the size checks every plan starts with.  The frame, tile, relief and final kernels, the plans and their caps are the
// callers'.  (avgpow.hip has one (T,) signal and shares framed.h alone.)
//
// As in framed.h, inlining is left to the compiler: no attribute asks for it here.
#pragma once
#include "framed.h"

namespace fl {
namespace framed {

// element strides of a (B, T, N) signal: the kernels read the signals as they lie
struct Strides {
    long b, t, c;
};

// the mel basis on the device: idx = start[NM], count[NM], offset[NM] (band j holds the bins start .. start + count - 1, its
// weights at w[offset ..]), then band[n_fft/2 + 1] (bin k lies in the bands band[k] and band[k] + 1 only);
// w = the nnz packed weights, then the two weights of every bin
struct Mel {
    const int* idx;
    const double* w;
    int nnz;
};

__device__ inline double power(cx<double> x) { return x.x * x.x + x.y * x.y; }

__device__ inline double sign(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0); }

// first element of row = b N + c of a signal (the plan's N channels)
template <class Plan>
__device__ inline long row_offset(const Plan& p, long row, Strides s) {
    const long b = row / p.N, c = row - b * p.N;
    return b * s.b + c * s.c;
}

// band j of the NM bands, from the |X|^2 of the NC + 1 bins in Sp; the table's entries are clamped to the arrays they index
template <int NC, int NM>
__device__ inline double mel_project(const double* Sp, const Mel& mel, int j) {
    const int start = min(max(mel.idx[j], 0), NC);
    int count = min(max(mel.idx[NM + j], 0), NC + 1 - start);
    const int off = mel.idx[2 * NM + j];
    if (off < 0 || off > mel.nnz - count) count = 0;
    const double* w = mel.w + off;
    const double* s = Sp + start;
    double a0 = 0.0, a1 = 0.0;
    int i = 0;
    for (; i + 1 < count; i += 2) {
        a0 = fma(w[i], s[i], a0);
        a1 = fma(w[i + 1], s[i + 1], a1);
    }
    if (i < count) a0 = fma(w[i], s[i], a0);
    return a0 + a1;
}

// 1 where the target's entry (a band energy, a magnitude) stands `threshold` dB over the noise energy, else 0 (a NaN keeps its
// entry, as the comparison SNR < threshold of the definition does)
template <class Opt>
__device__ inline double snr_mask(double mt, const Opt& o) {
    if (!o.apply_mask) return 1.0;
    const double snr = 10.0 * log10(fmax(mt * mt, o.ne * 1.01) - o.ne) - 10.0 * log10(o.ne);
    return snr < o.threshold ? 0.0 : 1.0;
}

// Runs body(0, .) and then body(1, .) as ONE loop body that is not unrolled, and hands back the NB values each left: the
// first signal's in `first`, the second's in `second`.  A prediction equal to the target must give band energies equal to
// the bit -- the loss and, for the 1-norm, sign(m_t - m_p) are exact zeros then -- and two inlined copies of the same
// source are not held to that: where a product is fused into an addition is decided copy by copy.
template <int NB, class Body>
__device__ inline void both_signals(double (&first)[NB], double (&second)[NB], Body&& body) {
#pragma clang loop unroll(disable)
    for (int sig = 0; sig < 2; ++sig) {
        if (sig) {
#pragma unroll
            for (int i = 0; i < NB; ++i) first[i] = second[i];
        }
        body(sig, second);
    }
}

// ---------------------------------------------------------------- combine: one workgroup per resolution, a fixed order
// where the partial sums of a resolution lie: `count` records of NSUM doubles from record `first` (filled by the host entry)
struct Spans {
    long first[8], count[8];
};

template <class Plan, class First, class Count>
inline Spans spans_of(const Plan& p, First&& first, Count&& count) {
    static_assert(std::extent<decltype(Plan::r)>::value <= 8, "Spans holds eight resolutions");
    Spans s{};
    for (int r = 0; r < p.R; ++r) {
        s.first[r] = first(p.r[r]);
        s.count[r] = count(p.r[r]);
    }
    return s;
}

// keep[KEEP_STRIDE r + c] = sum c of resolution r = blockIdx.x: stride-256 accumulation, the wavefronts' sums, then
// (0 + 1) + (2 + 3) -- no atomics, two runs give the same bits
template <int NSUM, int KEEP_STRIDE>
__global__ void __launch_bounds__(256) combine_kernel(const double* __restrict__ partial, Spans sp, double* __restrict__ keep) {
    __shared__ double red[NSUM][4];
    const int r = blockIdx.x;
    const long n = sp.count[r];
    const double* q = partial + NSUM * sp.first[r];
    double s[NSUM] = {};
    for (long i = threadIdx.x; i < n; i += 256) {
#pragma unroll
        for (int c = 0; c < NSUM; ++c) s[c] += q[NSUM * i + c];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NSUM; ++c) {
        s[c] = wave_sum(s[c]);
        if (lane == 0) red[c][wave] = s[c];
    }
    __syncthreads();
    if (threadIdx.x < NSUM) keep[KEEP_STRIDE * r + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// ---------------------------------------------------------------- overlap-add: a gather per sample, in a fixed order
// one thread per sample of gy (B, T, N), for a plan of p.R resolutions p.r[]: resolution by resolution, frame by frame
// (gather_sample), with the reflected margins folded back onto the interior samples they mirror
template <typename T, class Plan>
__global__ void __launch_bounds__(256) ola_kernel(const T* __restrict__ gframes, Plan p, const T* __restrict__ gloss, T* __restrict__ gy) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= p.rows * p.T) return;
    const long row = e / p.T, t = e - row * p.T;
    double acc = 0.0;
    for (int r = 0; r < p.R; ++r) {
        const auto& q = p.r[r];
        const T* g = gframes + q.g0 + row * q.F * q.win;
        gather_sample(g, t, p.T, q.nfft / 2, q, q.F - 1, acc);
    }
    const long b = row / p.N, c = row - b * p.N;
    gy[(b * p.T + t) * p.N + c] = (T)((double)gloss[0] * acc);
}

// ---------------------------------------------------------------- host: the checks every plan starts with
// 1 <= B, N, 1 <= T <= 2^30 and at most `samples_max` samples in all
inline bool signal_sizes(long B, long T, long N, long samples_max) {
    if (B < 1 || N < 1 || T < 1 || T > (1L << 30)) return false;
    return B <= samples_max / T && B * T <= samples_max / N;
}

// F = 1 + T / hop frames in a row (reflect padding by n_fft / 2 on both sides), or -1 when `rows` rows hold more than `most`
inline long frames_per_row(long T, int hop, long rows, long most) {
    const long F = 1 + T / hop;
    return F > most / rows ? -1 : F;
}

}  // namespace framed
}  // namespace fl
