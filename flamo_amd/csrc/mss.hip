// Linear multi-scale spectral criterion (gfx950 / MI355X): for each resolution n_fft (hop = its share of n_fft, the window the
// periodic Hann of n_fft samples) the magnitude spectrograms M = |X| of prediction and target on nnAudio's "linear" frequency
// scale -- K = n_fft / 2 + 1 analysis frequencies from 20 Hz, spaced slightly under one DFT bin, so bin k sits at the
// FRACTIONAL position beta_k = a + k s -- a mask from the target's signal-to-noise ratio, and the plain, the "yamamoto" or the
// "magenta" form of |(M_t - M_p) mask| and |(log M_t - log M_p) mask|; the loss is the SUM over the resolutions
// (include/flamo_hip_mss.h has the definition in full).
//
// The transform is no FFT: it is the dense product X[f, k] = sum_j A[f, j] E[j, k] of the windowed frames A (real) against
// E[j, k] = exp(-i theta_k j), theta_k = 2 pi beta_k / n_fft, on the float64 matrix cores: v_mfma_f64_16x16x4_f64 with frames
// as rows and bins as columns, the real and the imaginary part two accumulator sets.  A wavefront holds FWD_TILES bin tiles, so
// one A fragment (one LDS read) feeds 2 FWD_TILES instructions.  E is never stored (134 MB at 4096): a lane owns one bin per
// tile and the sample offset lane >> 4, and advances its E[j, k] by four samples with one complex product by exp(-4 i theta_k);
// every RESEED = 16 steps (64 samples, one staged chunk of A) it starts again from exp(-i theta_k 64 m), a host table whose
// phases are reduced in integers before the one float64 cosine (2 MB at 4096).  A run of 16 rotations stays within 2.7e-14 of
// the basis (derived; 1.7e-14 measured: tests/test_mss_host.py) -- the step's own rounding enters 15 times.
//
// Launches: THREE forward (tiles, combine, final) and TWO backward (adjoint tiles, overlap-add), whatever the list of
// resolutions, B, N, T and the data.  Both tile grids list the (resolution, row, 16 frames, bin or sample group) workgroups
// with the longest resolutions first: the time of a workgroup grows with n_fft.
//
// Forward tiles.  A workgroup of four wavefronts takes 16 frames x 256 bins; the frames' windowed samples are staged 64 at a
// time in LDS (two buffers: the next chunk is loaded while this one is multiplied, one barrier per chunk) straight from the
// signal through its strides and the reflection.  Prediction and target run through ONE loop body (`both_signals` of
// criterion.h): equal signals give equal M to the bit, and an exact 0 for the loss and every sign.  With `planes` the
// prediction's X and the target's M go to `keep` -- recomputing an O(n^2) transform in the backward pass would triple its
// work.  A workgroup leaves six sums; the combine is criterion.h's, the final kernel as in melmss.hip.
//
// Adjoint tiles.  A workgroup takes 16 frames x 512 samples of the frame; G = dL/dM_p X_p / M_p (0 where M_p is 0) is formed
// from the kept planes 64 bins at a time in LDS, and gframe[f, j] = w_j sum_k (Re G cos(theta_k j) - Im G sin(theta_k j)) runs
// on the same instruction with the bins as the contracted index: a lane owns one sample per tile and the bin offset lane >> 4,
// advances by four bins with exp(+i (theta_4 - theta_0) j) and starts again every 64 bins from exp(+i theta_{64 m} j).  The
// overlap-add is criterion.h's, framed::gather_sample per sample.
//
// Precision.  As in mrstft.hip, edr.hip and melmss.hip: the signals, the frame gradients and the gradient have the signals'
// type, everything between is a double in float32 too.
//
// Resources (the compiler's report for gfx950 is in DESIGN 4.6): LDS 17.5 KB forward, 35 KB backward; no scratch.
#include "criterion.h"
#include "../../include/flamo_hip_mss.h"

#include <math.h>

namespace fl {
namespace mss {

using C = double;
typedef double d4m __attribute__((ext_vector_type(4)));

constexpr int MAXR = 8, NFFT_MIN = 16, NFFT_MAX = 4096;
constexpr int NT = 256, FT = 16, CHUNK = 64, RESEED = CHUNK / 4, PAD = 4;
constexpr int FWD_TILES = 4, FWD_BINS = 4 * 16 * FWD_TILES;           // bins of a forward workgroup
constexpr int BWD_TILES = 8, BWD_SAMPLES = 4 * 16 * BWD_TILES;        // samples of an adjoint workgroup
// every launch stays under 2^32 threads (a grid of more has been refused by the runtime): the tile grids have at most 2^24 - 1
// workgroups of 256, the overlap-add one thread per sample.  (Far beyond any memory: 2^24 tiles keep over 100 GB of planes.)
constexpr long FRAMES_MAX = (1L << 31) - 1, BLOCKS_MAX = (1L << 24) - 1, SAMPLES_MAX = (1L << 32) - 256;
constexpr int NSUM = 6;      // sum mask d^2, sum mask |d|, the same two of the log difference, sum mask, sum M_t^2
constexpr int KEEP_STRIDE = 8, KEEP_C0 = 6, KEEP_C1 = 7, KEEP_LOSS = KEEP_STRIDE * MAXR, KEEP_HEAD = KEEP_LOSS + 1;

using framed::Strides;
using framed::sign;
using framed::row_offset;
using framed::snr_mask;      // (of a magnitude here)
using framed::both_signals;

struct Res : framed::Frame {
    int nfft, K, NJ, NK;     // bins, chunks of 64 samples, chunks of 64 bins
    int kg, jg;              // bin groups of the forward grid, sample groups of the adjoint grid
    long F, ft;              // frames per row, frame tiles per row
    long blk0, nblk;         // first workgroup and workgroups in the forward grid
    long bblk0;              // first workgroup in the adjoint grid
    long g0;                 // first element in gframes
    long t0;                 // first double in the tables
    long p0;                 // first double of the planes behind the head of keep
};
struct Plan {
    int R;
    long B, T, N, rows, frames, gelems, blocks, bblocks, tabdoubles, planedoubles;
    Res r[MAXR];
};
struct Opt {
    int lin_norm, log_norm, apply_mask, form;      // log_norm 0: no log term
    double alpha, threshold, ne;
};

// the part of a plan that the list of resolutions alone decides
static bool make_tables(int R, const int* res, Plan& p) {
    if (!res || R < 1 || R > MAXR) return false;
    p.R = R;
    long t = 0;
    for (int r = 0; r < R; ++r) {
        const int nfft = res[2 * r], hop = res[2 * r + 1];
        if (nfft < NFFT_MIN || nfft > NFFT_MAX || (nfft & 3) || hop < 1) return false;
        Res& q = p.r[r];
        q.nfft = nfft; q.hop = hop; q.win = nfft; q.lpad = 0;
        q.K = nfft / 2 + 1;
        q.NJ = (nfft + CHUNK - 1) / CHUNK;
        q.NK = (q.K + CHUNK - 1) / CHUNK;
        q.kg = (q.K + FWD_BINS - 1) / FWD_BINS;
        q.jg = (nfft + BWD_SAMPLES - 1) / BWD_SAMPLES;
        q.t0 = t;
        t += nfft + 2L * q.K * q.NJ + 2L * q.K * 5 + 2L * nfft * q.NK + 2L * nfft * 5;
    }
    p.tabdoubles = t;
    return true;
}

static bool make_plan(long B, long T, long N, int R, const int* res, Plan& p) {
    if (!make_tables(R, res, p) || !framed::signal_sizes(B, T, N, SAMPLES_MAX)) return false;
    p.B = B; p.T = T; p.N = N; p.rows = B * N;
    long frames = 0, g = 0, planes = 0;
    for (int r = 0; r < R; ++r) {
        Res& q = p.r[r];
        if (T <= q.nfft / 2) return false;
        q.F = framed::frames_per_row(T, q.hop, p.rows, FRAMES_MAX);
        if (q.F < 0) return false;
        q.ft = (q.F + FT - 1) / FT;
        q.g0 = g; q.p0 = planes;
        frames += p.rows * q.F;
        if (frames > FRAMES_MAX) return false;
        g += p.rows * q.F * q.nfft;
        planes += 3 * p.rows * q.F * q.K;
    }
    // the workgroups, longest frames first: the time of one grows with n_fft, and started last it would be the tail
    long blocks = 0, bblocks = 0;
    for (int nfft = NFFT_MAX; nfft >= NFFT_MIN; nfft -= 4)
        for (int r = 0; r < R; ++r) {
            Res& q = p.r[r];
            if (q.nfft != nfft) continue;
            q.blk0 = blocks; q.bblk0 = bblocks;
            q.nblk = p.rows * q.ft * q.kg;
            blocks += q.nblk;
            bblocks += p.rows * q.ft * q.jg;
            if (blocks > BLOCKS_MAX || bblocks > BLOCKS_MAX) return false;
        }
    p.frames = frames; p.gelems = g; p.blocks = blocks; p.bblocks = bblocks; p.planedoubles = planes;
    return true;
}

// (resolution, row, frame tile, group) of a workgroup: the resolution that starts last at or before it
template <bool BWD>
__device__ inline void locate(const Plan& p, long blk, int& r, long& row, long& ft, int& grp) {
    r = 0;
    long best = -1;
    for (int i = 0; i < p.R; ++i) {
        const long b0 = BWD ? p.r[i].bblk0 : p.r[i].blk0;
        if (blk >= b0 && b0 > best) {
            r = i;
            best = b0;
        }
    }
    const Res& q = p.r[r];
    const int groups = BWD ? q.jg : q.kg;
    const long local = blk - best, tile = local / groups;
    grp = (int)(local - tile * groups);
    row = tile / q.ft;
    ft = tile - row * q.ft;
}

// |X|, the same instructions wherever it is formed: the forward pass keeps M_t and the backward pass forms M_p again from the
// kept X_p, and for equal signals the two must be equal to the bit
__device__ inline double magnitude(double re, double im) { return sqrt(fma(re, re, im * im)); }

// ---------------------------------------------------------------- forward: 16 frames x 256 bins per workgroup
template <typename T>
__global__ void __launch_bounds__(NT)
mss_tile_kernel(const T* __restrict__ yp, Strides sp, const T* __restrict__ yt, Strides st, Plan p, const double* __restrict__ tab,
                Opt o, int planes, double* __restrict__ partial, double* __restrict__ keep) {
    __shared__ double As[2][FT][CHUNK + PAD];
    __shared__ double red[NSUM][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    int r, kgrp;
    long row, ft;
    locate<false>(p, blockIdx.x, r, row, ft, kgrp);
    const Res& q = p.r[r];
    const int n = q.nfft, K = q.K, NJ = q.NJ, half = n / 2;
    const long F = q.F, f0 = ft * FT;
    const int kb = kgrp * FWD_BINS + wave * (16 * FWD_TILES);
    const bool active = kb < K;      // (a wavefront without a bin still stages and meets the barriers)
    const double* w = tab + q.t0;
    const cx<C>* fseed = reinterpret_cast<const cx<C>*>(w + n);
    const cx<C>* fstep = fseed + (long)K * NJ;
    int kk[FWD_TILES];
    cx<C> step[FWD_TILES], off[FWD_TILES];
#pragma unroll
    for (int t = 0; t < FWD_TILES; ++t) {
        kk[t] = min(kb + 16 * t + li, K - 1);
        step[t] = fstep[kk[t] * 5 + 4];
        off[t] = fstep[kk[t] * 5 + lk];
    }
    const T* rows[2] = {yp + row_offset(p, row, sp), yt + row_offset(p, row, st)};
    const long strides[2] = {sp.t, st.t};
    double* plane = keep + KEEP_HEAD + q.p0;
    const long psize = p.rows * F * K;

    double mp[4 * FWD_TILES], mt[4 * FWD_TILES];
    both_signals<4 * FWD_TILES>(mp, mt, [&](int sig, double (&m)[4 * FWD_TILES]) {
        const T* y = rows[sig];
        const long stride = strides[sig];
        // 64 samples of the 16 windowed frames, loaded before the chunk in flight is multiplied and laid into LDS behind it;
        // what lies beyond the last frame or the last sample is 0
        constexpr int NS = FT * CHUNK / NT;
        double sv[NS];
        auto stage_load = [&](int c) {
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int e = tid + NT * i, f = e >> 6, j = CHUNK * c + (e & 63);
                const long fr = f0 + f;
                sv[i] = 0.0;
                if (fr < F && j < n) sv[i] = w[j] * (double)framed::padded(y, stride, p.T, fr * q.hop + j, half);
            }
        };
        auto stage_store = [&](int buf) {
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int e = tid + NT * i;
                As[buf][e >> 6][e & 63] = sv[i];
            }
        };
        d4m are[FWD_TILES], aim[FWD_TILES];
#pragma unroll
        for (int t = 0; t < FWD_TILES; ++t) are[t] = aim[t] = d4m{0.0, 0.0, 0.0, 0.0};
        stage_load(0);
        stage_store(0);
        // (the seeds of a chunk are fetched one chunk ahead, like its samples: a round trip to L2 per chunk would stand in
        // front of every run of 16 steps)
        cx<C> seed[FWD_TILES];
#pragma unroll
        for (int t = 0; t < FWD_TILES; ++t) seed[t] = fseed[(long)kk[t] * NJ];
        __syncthreads();
#pragma clang loop unroll(disable)
        for (int c = 0; c < NJ; ++c) {
            cx<C> ph[FWD_TILES];
#pragma unroll
            for (int t = 0; t < FWD_TILES; ++t) ph[t] = mul_plain(seed[t], off[t]);
            if (c + 1 < NJ) {
                stage_load(c + 1);
#pragma unroll
                for (int t = 0; t < FWD_TILES; ++t) seed[t] = fseed[(long)kk[t] * NJ + c + 1];
            }
            if (active) {
                const double* a = &As[c & 1][li][lk];
#pragma unroll 4
                for (int s = 0; s < RESEED; ++s) {
                    const double av = a[4 * s];
#pragma unroll
                    for (int t = 0; t < FWD_TILES; ++t) {
                        are[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, ph[t].x, are[t], 0, 0, 0);
                        aim[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, ph[t].y, aim[t], 0, 0, 0);
                        ph[t] = mul_plain(ph[t], step[t]);
                    }
                }
            }
            if (c + 1 < NJ) stage_store((c + 1) & 1);
            __syncthreads();
        }
#pragma unroll
        for (int t = 0; t < FWD_TILES; ++t) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const double re = are[t][rr], im = aim[t][rr], M = magnitude(re, im);
                m[4 * t + rr] = M;
                const int k = kb + 16 * t + li;
                const long f = f0 + lk + 4 * rr;
                if (planes && k < K && f < F) {
                    const long idx = (row * F + f) * K + k;
                    if (sig == 0) {
                        plane[idx] = re;
                        plane[psize + idx] = im;
                    } else {
                        plane[2 * psize + idx] = M;
                    }
                }
            }
        }
    });

    double s[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < FWD_TILES; ++t) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int k = kb + 16 * t + li;
            const long f = f0 + lk + 4 * rr;
            if (k < K && f < F) {
                const double Mt = mt[4 * t + rr], Mp = mp[4 * t + rr];
                const double mask = snr_mask(Mt, o);
                const double d = (Mt - Mp) * mask;
                s[0] += d * d;
                s[1] += fabs(d);
                if (o.log_norm) {
                    const double dl = (log(Mt) - log(Mp)) * mask;
                    s[2] += dl * dl;
                    s[3] += fabs(dl);
                }
                s[4] += mask;
                s[5] += Mt * Mt;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NSUM; ++c) s[c] = wave_sum(s[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NSUM; ++c) red[c][wave] = s[c];
    }
    __syncthreads();
    if (tid < NSUM) partial[NSUM * (long)blockIdx.x + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// one thread: the loss and, per resolution, the factors of dL/dM_p = -mask (c0 gd + c1 gl / M_p), gd = d under a 2-norm and
// sign d under a 1-norm, gl the same of dl (a 2-norm's gradient is 0 where the norm is, as torch's is)
template <typename T>
__global__ void __launch_bounds__(64) mss_final_kernel(Plan p, Opt o, double* __restrict__ keep, T* __restrict__ loss) {
    if (threadIdx.x != 0) return;
    double l = 0.0;
    for (int r = 0; r < p.R; ++r) {
        double* k = keep + KEEP_STRIDE * r;
        const double numel = (double)p.rows * (double)p.r[r].F * (double)p.r[r].K;
        double c0, c1 = 0.0;
        if (o.form == 0) {
            const double Nn = o.apply_mask ? k[4] : numel;
            const bool fro = o.lin_norm == 2;
            const double lin = fro ? sqrt(k[0]) : k[1];
            l += lin / Nn;
            c0 = fro ? (k[0] > 0.0 ? 1.0 / (lin * Nn) : 0.0) : 1.0 / Nn;
            if (o.log_norm) {
                const double lg = fro ? sqrt(k[2]) : k[3];
                l += o.alpha * lg / Nn;
                c1 = fro ? (k[2] > 0.0 ? o.alpha / (lg * Nn) : 0.0) : o.alpha / Nn;
            }
        } else if (o.form == 1) {
            const double lin = sqrt(k[0]), den = sqrt(k[5]);
            l += lin / den + o.alpha * k[3] / numel;
            c0 = k[0] > 0.0 ? 1.0 / (lin * den) : 0.0;
            c1 = o.alpha / numel;
        } else {
            l += (k[1] + o.alpha * k[3]) / numel;
            c0 = 1.0 / numel;
            c1 = o.alpha / numel;
        }
        k[KEEP_C0] = c0;
        k[KEEP_C1] = c1;
    }
    keep[KEEP_LOSS] = l;
    loss[0] = (T)l;
}

// ---------------------------------------------------------------- backward: 16 frames x 512 samples per workgroup
template <typename T>
__global__ void __launch_bounds__(NT)
mss_adjoint_kernel(Plan p, const double* __restrict__ tab, Opt o, const double* __restrict__ keep, T* __restrict__ gframes) {
    __shared__ double Gs[2][2][FT][CHUNK + PAD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    int r, jgrp;
    long row, ft;
    locate<true>(p, blockIdx.x, r, row, ft, jgrp);
    const Res& q = p.r[r];
    const int n = q.nfft, K = q.K, NK = q.NK;
    const long F = q.F, f0 = ft * FT;
    const int jb = jgrp * BWD_SAMPLES + wave * (16 * BWD_TILES);
    const bool active = jb < n;
    const double* w = tab + q.t0;
    const cx<C>* bseed = reinterpret_cast<const cx<C>*>(w + n) + (long)K * q.NJ + (long)K * 5;
    const cx<C>* bstep = bseed + (long)n * NK;
    const double c0 = keep[KEEP_STRIDE * r + KEEP_C0], c1 = keep[KEEP_STRIDE * r + KEEP_C1];
    const double* plane = keep + KEEP_HEAD + q.p0;
    const long psize = p.rows * F * K;
    int jj[BWD_TILES];
    cx<C> step[BWD_TILES], off[BWD_TILES];
#pragma unroll
    for (int t = 0; t < BWD_TILES; ++t) {
        jj[t] = min(jb + 16 * t + li, n - 1);
        step[t] = bstep[jj[t] * 5 + 4];
        off[t] = bstep[jj[t] * 5 + lk];
    }
    // G = dL/dM_p X_p / M_p of 64 bins of the 16 frames; 0 where M_p is, under the mask, and beyond the last frame or bin.  The
    // kept values are loaded before the chunk in flight is multiplied; G is formed and laid into LDS behind it.
    constexpr int NS = FT * CHUNK / NT;
    double sxr[NS], sxi[NS], smt[NS];
    auto stage_load = [&](int c) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int e = tid + NT * i, f = e >> 6, k = CHUNK * c + (e & 63);
            const long fr = f0 + f;
            sxr[i] = sxi[i] = smt[i] = 0.0;
            if (fr < F && k < K) {
                const long idx = (row * F + fr) * K + k;
                sxr[i] = plane[idx];
                sxi[i] = plane[psize + idx];
                smt[i] = plane[2 * psize + idx];
            }
        }
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int e = tid + NT * i;
            const double xr = sxr[i], xi = sxi[i], Mt = smt[i];
            const double Mp = magnitude(xr, xi);
            double gr = 0.0, gi = 0.0;
            if (Mp != 0.0 && snr_mask(Mt, o) != 0.0) {
                const double d = Mt - Mp;
                double g = c0 * (o.lin_norm == 2 ? d : sign(d));
                if (o.log_norm) {
                    const double dl = log(Mt) - log(Mp);
                    g += c1 * (o.log_norm == 2 ? dl : sign(dl)) / Mp;
                }
                g = -g / Mp;
                gr = g * xr;
                gi = g * xi;
            }
            Gs[buf][0][e >> 6][e & 63] = gr;
            Gs[buf][1][e >> 6][e & 63] = gi;
        }
    };
    d4m acc[BWD_TILES];
#pragma unroll
    for (int t = 0; t < BWD_TILES; ++t) acc[t] = d4m{0.0, 0.0, 0.0, 0.0};
    stage_load(0);
    stage_store(0);
    cx<C> seed[BWD_TILES];      // (fetched one chunk ahead, as in the forward kernel)
#pragma unroll
    for (int t = 0; t < BWD_TILES; ++t) seed[t] = bseed[(long)jj[t] * NK];
    __syncthreads();
#pragma clang loop unroll(disable)
    for (int c = 0; c < NK; ++c) {
        cx<C> ph[BWD_TILES];
#pragma unroll
        for (int t = 0; t < BWD_TILES; ++t) ph[t] = mul_plain(seed[t], off[t]);
        if (c + 1 < NK) {
            stage_load(c + 1);
#pragma unroll
            for (int t = 0; t < BWD_TILES; ++t) seed[t] = bseed[(long)jj[t] * NK + c + 1];
        }
        if (active) {
            const double* ar = &Gs[c & 1][0][li][lk];
            const double* ai = &Gs[c & 1][1][li][lk];
#pragma unroll 2
            for (int s = 0; s < RESEED; ++s) {
                const double vr = ar[4 * s], vi = ai[4 * s];
#pragma unroll
                for (int t = 0; t < BWD_TILES; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(vr, ph[t].x, acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < BWD_TILES; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(vi, -ph[t].y, acc[t], 0, 0, 0);
                    ph[t] = mul_plain(ph[t], step[t]);
                }
            }
        }
        if (c + 1 < NK) stage_store((c + 1) & 1);
        __syncthreads();
    }
    T* out = gframes + q.g0 + row * F * n;
#pragma unroll
    for (int t = 0; t < BWD_TILES; ++t) {
        const int j = jb + 16 * t + li;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const long f = f0 + lk + 4 * rr;
            if (j < n && f < F) out[f * n + j] = (T)(w[j] * acc[t][rr]);
        }
    }
}

}  // namespace mss
}  // namespace fl

using namespace fl;
using namespace fl::mss;

extern "C" long fl_mss_frames(long B, long T, long N, int R, int* res) {
    Plan p;
    return make_plan(B, T, N, R, res, p) ? p.frames : -1;
}
extern "C" long fl_mss_partial_doubles(long B, long T, long N, int R, int* res) {
    Plan p;
    return make_plan(B, T, N, R, res, p) ? NSUM * p.blocks : -1;
}
extern "C" long fl_mss_keep_doubles(long B, long T, long N, int R, int* res, int planes) {
    Plan p;
    return make_plan(B, T, N, R, res, p) ? KEEP_HEAD + (planes ? p.planedoubles : 0) : -1;
}
extern "C" long fl_mss_gframe_elems(long B, long T, long N, int R, int* res) {
    Plan p;
    return make_plan(B, T, N, R, res, p) ? p.gelems : -1;
}
extern "C" long fl_mss_table_doubles(int R, int* res) {
    Plan p;
    return make_tables(R, res, p) ? p.tabdoubles : -1;
}
extern "C" long fl_mss_launches(int R, int* res, int backward) {
    Plan p;
    if (!make_tables(R, res, p)) return -1;
    return backward ? 2 : 3;
}

#define FL_MSS_PLAN(who)                                                                                                         \
    Plan p;                                                                                                                      \
    FL_REQUIRE(make_plan(B, Tn, N, R, res, p),                                                                                   \
               who ": bad sizes (1 <= R <= 8 resolutions (n_fft, hop), n_fft a multiple of 4 from 16 to 4096, hop >= 1, "        \
                   "n_fft / 2 < T <= 2^30, fewer than 2^31 frames, 2^24 workgroups per launch and 2^32 samples in all)");                            \
    FL_REQUIRE(norm == 1 || norm == 2, who ": norm must be 1 or 2");                                                             \
    FL_REQUIRE(form >= 0 && form <= 2, who ": form must be 0 (plain), 1 (yamamoto) or 2 (magenta)");                             \
    FL_REQUIRE(!apply_mask || (noise_energy > 0.0 && noise_energy < HUGE_VAL), who ": apply_mask needs a finite noise_energy > 0"); \
    FL_REQUIRE((uintptr_t)tab % (2 * sizeof(C)) == 0, who ": the tables must be aligned to their complex elements");             \
    const Opt o{form == 0 ? norm : (form == 1 ? 2 : 1), form == 0 ? (log_term ? norm : 0) : 1, apply_mask ? 1 : 0, form, alpha_, \
                threshold, noise_energy}

// (Tn: the header's T, the signals' length -- T is the precision here)
FL_ENTRY_F32_F64(fl_mss_fwd, (const void* yp, long spb, long spt, long spc, const void* yt, long stb, long stt, long stc, long B, long Tn,
                              long N, int R, int* res, const void* tab, int norm, int form, int log_term, double alpha, int apply_mask,
                              double threshold, double noise_energy, int planes, void* partial, void* keep, void* loss, void* stream),
                 (yp, spb, spt, spc, yt, stb, stt, stc, B, Tn, N, R, res, tab, norm, form, log_term, alpha, apply_mask, threshold,
                  noise_energy, planes, partial, keep, loss, stream)) {
    FL_REQUIRE(yp && yt && res && tab && partial && keep && loss, "mss_fwd: null pointer");
    const double alpha_ = alpha;
    FL_MSS_PLAN("mss_fwd");
    const Strides sp{spb, spt, spc}, st{stb, stt, stc};
    hipLaunchKernelGGL((mss_tile_kernel<T>), dim3((unsigned)p.blocks), dim3(NT), 0, (hipStream_t)stream, (const T*)yp, sp, (const T*)yt,
                       st, p, (const double*)tab, o, planes ? 1 : 0, (double*)partial, (double*)keep);
    FL_CHECK_LAUNCH("mss_tile");
    const framed::Spans sums = framed::spans_of(p, [](const Res& q) { return q.blk0; }, [](const Res& q) { return q.nblk; });
    hipLaunchKernelGGL((framed::combine_kernel<NSUM, KEEP_STRIDE>), dim3((unsigned)p.R), dim3(256), 0, (hipStream_t)stream,
                       (const double*)partial, sums, (double*)keep);
    FL_CHECK_LAUNCH("mss_combine");
    hipLaunchKernelGGL((mss_final_kernel<T>), dim3(1), dim3(64), 0, (hipStream_t)stream, p, o, (double*)keep, (T*)loss);
    FL_CHECK_LAUNCH("mss_final");
    return FL_OK;
}

FL_ENTRY_F32_F64(fl_mss_bwd, (long B, long Tn, long N, int R, int* res, const void* tab, int norm, int form, int log_term, int apply_mask,
                              double threshold, double noise_energy, const void* keep, const void* gloss, void* gframes, void* gy,
                              void* stream),
                 (B, Tn, N, R, res, tab, norm, form, log_term, apply_mask, threshold, noise_energy, keep, gloss, gframes, gy, stream)) {
    FL_REQUIRE(res && tab && keep && gloss && gframes && gy, "mss_bwd: null pointer");
    const double alpha_ = 0.0;      // (folded into keep by the forward entry)
    FL_MSS_PLAN("mss_bwd");
    hipLaunchKernelGGL((mss_adjoint_kernel<T>), dim3((unsigned)p.bblocks), dim3(NT), 0, (hipStream_t)stream, p, (const double*)tab, o,
                       (const double*)keep, (T*)gframes);
    FL_CHECK_LAUNCH("mss_adjoint");
    const long blocks = (p.rows * p.T + 255) / 256;
    hipLaunchKernelGGL((framed::ola_kernel<T, Plan>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const T*)gframes, p,
                       (const T*)gloss, (T*)gy);
    FL_CHECK_LAUNCH("mss_ola");
    return FL_OK;
}
