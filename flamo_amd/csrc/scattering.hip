// Scattering feedback matrices evaluated per bin in their factored form (gfx950 / MI355X).
//
//   H[f] = D(m_L) U_K D(m_K) ... U_1 D(m_1) U_0 D(m_R),    D(m) = diag(amp_i W_n^((f m_i) mod n))
//
// (ScatteringMatrix / VelvetNoiseMatrix, flamo/processor/dsp.py:1052-1348 over flamo/auxiliary/scattering.py:67-94, which
// convolves an (L, N, N) FIR matrix together and transforms it).  U_s are real N x N matrices, the delays are integers whose
// phase index is reduced in 64-bit integers and read from the master twiddle table as in the integer-delay response
// (response.hip); the amplitudes (alias envelope and per-sample gain raised to the delay) come from the caller in float64.
//
// Forward: one lane per (bin, input column).  The column's N-vector lives in registers and walks through the stages; the stage
// matrices, delays and amplitudes are wave-uniform.  Stores are contiguous along bins.
// Backward: the same lanes walk the cotangent column back through the stages; the lane's w_s = D(m_s) v_{s-1} is recomputed
// from the column's start (no per-stage (M, N, N) tensor exists anywhere).  dU_s = Re sum_lanes a_s w_s^H is formed per
// workgroup through LDS, accumulated in double into the workgroup's own row of `part`, and a second launch sums the rows in
// a fixed order: no atomics, the same bits every run.
#include "common.h"
#include "response_common.h"

namespace fl {

constexpr int kScatterMaxN = 32;
constexpr int kScatterMaxStages = 8;     // K + 1

// W_n^((k m) mod n), 0 <= m < n (the caller reduces the delay): the product is exact in double, the quotient estimate off by one
// at most (as delay_response_kernel); an index that still fell outside the table would be a caller's error and reads entry 0
template <typename T>
__device__ __forceinline__ cx<T> scatter_phase(const cx<T>* __restrict__ W, int nfft, double inv_nfft, int k, int m) {
    const long long prod = (long long)k * (long long)m;
    long long idx = prod - (long long)((double)prod * inv_nfft) * nfft;
    idx += (idx < 0) ? nfft : 0;
    idx -= (idx >= nfft) ? nfft : 0;
    if ((unsigned long long)idx >= (unsigned long long)nfft) idx = 0;
    return W[idx];
}

// v <- D(m) v  (conj_phase: D(m)^H v)
template <typename T, int NP>
__device__ __forceinline__ void scatter_diag(cx<T> (&v)[NP], const int32_t* __restrict__ m, const T* __restrict__ amp, int N,
                                             const cx<T>* __restrict__ W, int nfft, double inv_nfft, int k, bool conj_phase) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if (i < N) {
            cx<T> p = scatter_phase(W, nfft, inv_nfft, k, m[i]);
            if (conj_phase) p.y = -p.y;
            const T a = amp[i];
            const cx<T> x = v[i];
            v[i] = cx<T>(a * (x.x * p.x - x.y * p.y), a * (x.x * p.y + x.y * p.x));
        }
    }
}

// y = U x (transposed: U^T x), U real N x N row-major, wave-uniform
template <typename T, int NP>
__device__ __forceinline__ void scatter_matvec(const T* __restrict__ U, int N, const cx<T> (&x)[NP], cx<T> (&y)[NP], bool transposed) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        cx<T> acc((T)0, (T)0);
        if (i < N) {
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                if (j < N) {
                    const T u = transposed ? U[j * N + i] : U[i * N + j];
                    acc.x += u * x[j].x;
                    acc.y += u * x[j].y;
                }
            }
        }
        y[i] = acc;
    }
}

// v_0 = U_0[:, j] amp_R[j] phase(m_R[j])
template <typename T, int NP>
__device__ __forceinline__ void scatter_start(cx<T> (&v)[NP], const T* __restrict__ U0, int N, int j, const int32_t* __restrict__ mR,
                                              const T* __restrict__ ampR, const cx<T>* __restrict__ W, int nfft, double inv_nfft, int k) {
    const cx<T> p = scatter_phase(W, nfft, inv_nfft, k, mR[j]);
    const T a = ampR[j];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const T u = (i < N) ? U0[i * N + j] * a : (T)0;
        v[i] = cx<T>(u * p.x, u * p.y);
    }
}

struct ScatterArgs {
    const int32_t* sh;      // (K, N) stage delays
    const int32_t* mL;      // (N)
    const int32_t* mR;      // (N)
    int N, K, nfft, bin0, m_local;
    double inv_nfft;
};

template <typename T, int NP>
__global__ void __launch_bounds__(256) scatter_response_kernel(const T* __restrict__ U, const T* __restrict__ amp, const T* __restrict__ ampL,
                                                              const T* __restrict__ ampR, ScatterArgs g, const cx<T>* __restrict__ W,
                                                              cx<T>* __restrict__ H, long h_pitch) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= g.m_local) return;
    const int j = blockIdx.y, N = g.N, k = g.bin0 + f;
    cx<T> v[NP], t[NP];
    scatter_start<T, NP>(v, U, N, j, g.mR, ampR, W, g.nfft, g.inv_nfft, k);
    for (int s = 1; s <= g.K; ++s) {
        scatter_diag<T, NP>(v, g.sh + (s - 1) * N, amp + (s - 1) * N, N, W, g.nfft, g.inv_nfft, k, false);
        scatter_matvec<T, NP>(U + (size_t)s * N * N, N, v, t, false);
#pragma unroll
        for (int i = 0; i < NP; ++i) v[i] = t[i];
    }
    scatter_diag<T, NP>(v, g.mL, ampL, N, W, g.nfft, g.inv_nfft, k, false);
#pragma unroll
    for (int i = 0; i < NP; ++i)
        if (i < N) H[(size_t)(i * N + j) * h_pitch + f] = v[i];
}

// lanes of a backward workgroup: 32 KB of LDS for the two (NP, TB) tiles where 64 lanes allow it
template <typename T, int NP>
constexpr int scatter_bwd_lanes() {
    constexpr int fit = 32768 / (2 * NP * (int)sizeof(cx<T>));
    return fit >= 256 ? 256 : fit >= 128 ? 128 : 64;
}

template <typename T, int NP, int TB>
__global__ void __launch_bounds__(TB) scatter_response_bwd_kernel(const cx<T>* __restrict__ G, long g_pitch, const T* __restrict__ U,
                                                                 const T* __restrict__ amp, const T* __restrict__ ampL,
                                                                 const T* __restrict__ ampR, ScatterArgs g, const cx<T>* __restrict__ W,
                                                                 double* __restrict__ part, int n_bin_tiles) {
    __shared__ cx<T> la[NP * TB];      // [row][lane]
    __shared__ cx<T> lw[NP * TB];
    const int N = g.N, K = g.K, NN = N * N, tid = threadIdx.x;
    double* mine = part + (size_t)blockIdx.x * (size_t)(K + 1) * NN;
    const int n_tiles = n_bin_tiles * N;
    bool first = true;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, first = false) {
        const int j = tile / n_bin_tiles, f = (tile - j * n_bin_tiles) * TB + tid;
        const bool live = f < g.m_local;
        const int k = live ? g.bin0 + f : 0;
        cx<T> a[NP], v[NP], t[NP];
        // a_K = D(m_L)^H G[f, :, j]
#pragma unroll
        for (int i = 0; i < NP; ++i)
            a[i] = (live && i < N) ? G[(size_t)(i * N + j) * g_pitch + f] : cx<T>((T)0, (T)0);
        scatter_diag<T, NP>(a, g.mL, ampL, N, W, g.nfft, g.inv_nfft, k, true);
        for (int s = K; s >= 0; --s) {
            // w_s of this lane, from the column's start (s = 0: the unit vector e_j times the right delay)
            if (s > 0) {
                scatter_start<T, NP>(v, U, N, j, g.mR, ampR, W, g.nfft, g.inv_nfft, k);
                for (int q = 1; q < s; ++q) {
                    scatter_diag<T, NP>(v, g.sh + (q - 1) * N, amp + (q - 1) * N, N, W, g.nfft, g.inv_nfft, k, false);
                    scatter_matvec<T, NP>(U + (size_t)q * NN, N, v, t, false);
#pragma unroll
                    for (int i = 0; i < NP; ++i) v[i] = t[i];
                }
                scatter_diag<T, NP>(v, g.sh + (s - 1) * N, amp + (s - 1) * N, N, W, g.nfft, g.inv_nfft, k, false);
            } else {
                const cx<T> p = scatter_phase(W, g.nfft, g.inv_nfft, k, g.mR[j]);
                const T ar = ampR[j];
#pragma unroll
                for (int i = 0; i < NP; ++i) v[i] = (i == j) ? cx<T>(ar * p.x, ar * p.y) : cx<T>((T)0, (T)0);
            }
            __syncthreads();      // the previous stage's sums have been read
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                if (i < N) {
                    la[i * TB + tid] = a[i];
                    lw[i * TB + tid] = live ? v[i] : cx<T>((T)0, (T)0);
                }
            }
            __syncthreads();
            // dU_s[i][jj] += Re sum_lanes a[i] conj(w[jj]); each lane starts at its own offset (no two on one bank)
            for (int e = tid; e < NN; e += TB) {
                const int i = e / N, jj = e - i * N;
                const cx<T>* pa = la + i * TB;
                const cx<T>* pw = lw + jj * TB;
                double sum = 0.0;
                for (int l = 0; l < TB; ++l) {
                    const int ll = (l + tid) & (TB - 1);
                    const cx<T> x = pa[ll], y = pw[ll];
                    sum += (double)(x.x * y.x + x.y * y.y);
                }
                double* dst = mine + (size_t)s * NN + e;
                *dst = first ? sum : *dst + sum;      // this thread owns the entry: plain read-modify-write
            }
            // a_{s-1} = D(m_s)^H U_s^T a_s
            if (s > 0) {
                scatter_matvec<T, NP>(U + (size_t)s * NN, N, a, t, true);
#pragma unroll
                for (int i = 0; i < NP; ++i) a[i] = t[i];
                scatter_diag<T, NP>(a, g.sh + (s - 1) * N, amp + (s - 1) * N, N, W, g.nfft, g.inv_nfft, k, true);
            }
        }
    }
}

// dU[e] = sum over the workgroups' rows of part in a fixed order: 16 entries x 16 row groups per workgroup, thread (entry, group)
// adds rows group, group + 16, ... and the 16 group sums are added first to last (one thread per entry walking every row took
// 0.12 us a row: 190 us at 1536 rows)
template <typename T>
__global__ void __launch_bounds__(256) scatter_sum_parts_kernel(const double* __restrict__ part, int rows, int n, T* __restrict__ dU) {
    __shared__ double red[16][17];
    const int el = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + el;
    double s = 0.0;
    if (e < n)
        for (int r = grp; r < rows; r += 16) s += part[(size_t)r * n + e];
    red[grp][el] = s;
    __syncthreads();
    if (grp == 0 && e < n) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) t += red[q][el];
        dU[e] = (T)t;
    }
}

static inline int scatter_np(int N) { return N <= 2 ? 2 : N <= 4 ? 4 : N <= 8 ? 8 : N <= 16 ? 16 : 32; }

static inline bool scatter_sizes_ok(int N, int stages) {
    return N >= 2 && N <= kScatterMaxN && stages >= 2 && stages <= kScatterMaxStages;
}

template <typename T, int NP>
static int scatter_bwd_tiles(int m_local) { return cdiv_i(m_local, scatter_bwd_lanes<T, NP>()); }

// workgroups of the backward launch = rows of its scratch: every (bin tile, column) once, capped at six per compute unit (the
// kernel is bound by the latency of its dependent chains: it wants every wave slot its registers leave)
template <typename T>
static int scatter_bwd_blocks(int N, int m_local) {
    int tiles = 0;
    dispatch<2, 4, 8, 16, 32>(scatter_np(N), [&](auto np) { tiles = scatter_bwd_tiles<T, decltype(np)::value>(m_local); });
    const long total = (long)tiles * N, cap = 6L * device_cus();
    return (int)(total < cap ? (total > 0 ? total : 1) : cap);
}

}  // namespace fl

using namespace fl;

// ================================================================ the exported entries (C linkage), in the order of include/flamo_hip.h
extern "C" int fl_scatter_supported(int N, int stages) { return scatter_sizes_ok(N, stages) ? 1 : 0; }

FL_ENTRY_C64_C128(fl_scatter_response, (const void* U, const void* amp, const int32_t* shifts, const void* ampL, const int32_t* mL,
                                        const void* ampR, const int32_t* mR, int N, int stages, const void* W, int nfft, int bin0,
                                        int m_local, void* H, long h_pitch, void* stream),
                  (U, amp, shifts, ampL, mL, ampR, mR, N, stages, W, nfft, bin0, m_local, H, h_pitch, stream)) {
    FL_REQUIRE(U && amp && shifts && ampL && mL && ampR && mR && W && H, "scatter_response: null pointer");
    FL_REQUIRE(scatter_sizes_ok(N, stages), "scatter_response: 2 <= N <= 32 and 2 <= stages <= 8 (got N = %d, stages = %d)", N, stages);
    FL_REQUIRE(bin0 >= 0, "scatter_response: the row-major bin order is not generated here (permute the natural order)");
    FL_REQUIRE(nfft > 0 && nfft <= (1 << 26) && m_local >= 0 && (long)bin0 + m_local <= (long)nfft, "scatter_response: bad sizes");
    FL_REQUIRE(h_pitch >= m_local, "scatter_response: h_pitch must be >= m_local");
    if (m_local == 0) return FL_OK;
    const ScatterArgs g{shifts, mL, mR, N, stages - 1, nfft, bin0, m_local, 1.0 / (double)nfft};
    const dim3 grid(cdiv_i(m_local, 256), N);
    dispatch<2, 4, 8, 16, 32>(scatter_np(N), [&](auto np) {
        hipLaunchKernelGGL((scatter_response_kernel<T, decltype(np)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)U,
                           (const T*)amp, (const T*)ampL, (const T*)ampR, g, (const cx<T>*)W, (cx<T>*)H, h_pitch);
    });
    FL_CHECK_LAUNCH("scatter_response");
    return FL_OK;
}

extern "C" int fl_scatter_bwd_blocks(int N, int m_local, int is_f64) {
    if (N < 2 || N > kScatterMaxN || m_local < 0) return 0;
    return is_f64 ? scatter_bwd_blocks<double>(N, m_local) : scatter_bwd_blocks<float>(N, m_local);
}

FL_ENTRY_C64_C128(fl_scatter_response_bwd, (const void* G, long g_pitch, const void* U, const void* amp, const int32_t* shifts,
                                            const void* ampL, const int32_t* mL, const void* ampR, const int32_t* mR, int N, int stages,
                                            const void* W, int nfft, int bin0, int m_local, void* part, int part_rows, void* dU,
                                            void* stream),
                  (G, g_pitch, U, amp, shifts, ampL, mL, ampR, mR, N, stages, W, nfft, bin0, m_local, part, part_rows, dU, stream)) {
    FL_REQUIRE(G && U && amp && shifts && ampL && mL && ampR && mR && W && part && dU, "scatter_response_bwd: null pointer");
    FL_REQUIRE(scatter_sizes_ok(N, stages), "scatter_response_bwd: 2 <= N <= 32 and 2 <= stages <= 8 (got N = %d, stages = %d)", N, stages);
    FL_REQUIRE(bin0 >= 0, "scatter_response_bwd: the row-major bin order is not taken here (permute to the natural order)");
    FL_REQUIRE(nfft > 0 && nfft <= (1 << 26) && m_local >= 0 && (long)bin0 + m_local <= (long)nfft, "scatter_response_bwd: bad sizes");
    FL_REQUIRE(g_pitch >= m_local, "scatter_response_bwd: g_pitch must be >= m_local");
    const int blocks = scatter_bwd_blocks<T>(N, m_local);
    FL_REQUIRE(part_rows == blocks, "scatter_response_bwd: part must have fl_scatter_bwd_blocks = %d rows (got %d)", blocks, part_rows);
    const ScatterArgs g{shifts, mL, mR, N, stages - 1, nfft, bin0, m_local, 1.0 / (double)nfft};
    const int n = stages * N * N;
    // (m_local == 0: one workgroup with no tile writes nothing; the sum below must then see zeros)
    if (m_local == 0) {
        const int rc = check_hip(hipMemsetAsync(part, 0, (size_t)blocks * n * sizeof(double), (hipStream_t)stream), "scatter_response_bwd");
        if (rc) return rc;
    } else {
        dispatch<2, 4, 8, 16, 32>(scatter_np(N), [&](auto np) {
            constexpr int NP = decltype(np)::value;
            constexpr int TB = scatter_bwd_lanes<T, NP>();
            hipLaunchKernelGGL((scatter_response_bwd_kernel<T, NP, TB>), dim3(blocks), dim3(TB), 0, (hipStream_t)stream, (const cx<T>*)G,
                               g_pitch, (const T*)U, (const T*)amp, (const T*)ampL, (const T*)ampR, g, (const cx<T>*)W, (double*)part,
                               scatter_bwd_tiles<T, NP>(m_local));
        });
        FL_CHECK_LAUNCH("scatter_response_bwd");
    }
    hipLaunchKernelGGL((scatter_sum_parts_kernel<T>), dim3(cdiv_i(n, 16)), dim3(256), 0, (hipStream_t)stream, (const double*)part,
                       blocks, n, (T*)dU);
    FL_CHECK_LAUNCH("scatter_response_bwd (sum)");
    return FL_OK;
}
