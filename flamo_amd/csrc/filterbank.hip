// Frequency-domain band split (gfx950 / MI355X): the product of a spectrum with the responses of K Butterworth bands, the
// middle of the reference's FilterBank (flamo/auxiliary/filterbank.py:154-183: one rfft, a product per band, one irfft per
// band) between the library's own real transforms.
//
//   forward    Y[r, j, k] = H_j(w_k) X[r, k]                    w_k = pi k / M, k < M
//   backward   gX[r, k]   = sum_j conj(H_j(w_k)) gY[r, j, k]
//
// The responses are never stored: a thread evaluates H_j(w_k) from the band's zeros, poles and gain where it needs it, in the
// form about z = 1 and in double under either precision of the data (include/flamo_hip_filterbank.h says why).  Forward, a
// thread owns one (bin, band) and walks the rows with that one response; backward, a thread owns one bin of RB rows, walks the
// bands and keeps the RB band sums in registers (bands first to last: a fixed order).  Lanes are consecutive bins, so every
// load and store of a wavefront is one contiguous run of a row.
#include "common.h"
#include "../../include/flamo_hip_filterbank.h"

namespace fl {
namespace fbank {

constexpr int MAXP = FL_FILTERBANK_MAXP;
constexpr int BAND = FL_FILTERBANK_BAND;      // doubles of a band: nz, np, g, (unused), MAXP x (1 - z_i), MAXP x (1 - p_i)
constexpr int RB = 4;                         // rows of a backward thread
static_assert(BAND == 4 + 4 * MAXP, "the band record of include/flamo_hip_filterbank.h");

// u = z - 1 on the grid: -2 sin^2(w / 2) + i sin w, w = pi k / M
__device__ inline cx<double> grid_u(long k, long M) {
    double s, c;
    sincospi((double)k / (double)(2 * M), &s, &c);
    return cx<double>(-2.0 * s * s, 2.0 * s * c);
}

// g prod (u + (1 - z_i)) / prod (u + (1 - p_i)) of the band record at c
__device__ inline cx<double> band_response(const double* __restrict__ c, cx<double> u) {
    const int nz = min(max((int)c[0], 0), MAXP), np = min(max((int)c[1], 0), MAXP);
    const cx<double>* zc = reinterpret_cast<const cx<double>*>(c + 4);
    const cx<double>* pc = zc + MAXP;
    cx<double> num(c[2], 0.0), den(1.0, 0.0);
    for (int i = 0; i < nz; ++i) num = num * (u + zc[i]);
    for (int i = 0; i < np; ++i) den = den * (u + pc[i]);
    return cdiv(num, den);
}

template <typename T>
__global__ void __launch_bounds__(256) fbank_fwd_kernel(const cx<T>* __restrict__ X, long pitch_x, long rows, long M,
                                                        const double* __restrict__ consts, int K, cx<T>* __restrict__ Y,
                                                        long pitch_y) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    if (k >= M || j >= K) return;
    const cx<double> Hd = band_response(consts + (long)j * BAND, grid_u(k, M));
    const cx<T> H((T)Hd.x, (T)Hd.y);
    const cx<T>* x = X + k;
    cx<T>* y = Y + (long)j * pitch_y + k;
    for (long r = 0; r < rows; ++r) y[r * K * pitch_y] = x[r * pitch_x] * H;
}

template <typename T>
__global__ void __launch_bounds__(256) fbank_bwd_kernel(const cx<T>* __restrict__ gY, long pitch_y, long rows, long M,
                                                        const double* __restrict__ consts, int K, cx<T>* __restrict__ gX,
                                                        long pitch_x) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    const long r0 = (long)blockIdx.y * RB;
    if (k >= M || r0 >= rows) return;
    const int nr = (int)min((long)RB, rows - r0);
    const cx<double> u = grid_u(k, M);
    cx<T> acc[RB];
#pragma unroll
    for (int q = 0; q < RB; ++q) acc[q] = cx<T>((T)0, (T)0);
    for (int j = 0; j < K; ++j) {
        const cx<double> Hd = band_response(consts + (long)j * BAND, u);
        const cx<T> H((T)Hd.x, (T)Hd.y);
#pragma unroll
        for (int q = 0; q < RB; ++q)
            if (q < nr) fma_cxc(acc[q], gY[((r0 + q) * K + j) * pitch_y + k], H);
    }
#pragma unroll
    for (int q = 0; q < RB; ++q)
        if (q < nr) gX[(r0 + q) * pitch_x + k] = acc[q];
}

#define FL_FBANK_SIZES(who)                                                                                        \
    FL_REQUIRE(fl_filterbank_supports(K, 0), who ": 1 to %d bands, got %d", FL_FILTERBANK_MAXK, K);                \
    FL_REQUIRE(rows >= 1 && M >= 1 && M <= (1L << 30), who ": bad sizes (rows >= 1, 1 <= M <= 2^30)");             \
    FL_REQUIRE(pitch_x >= M && pitch_y >= M, who ": rows need a pitch >= M");                                      \
    FL_REQUIRE(rows * K < (1L << 31) && (rows + RB - 1) / RB <= 65535, who ": too many rows")

}  // namespace fbank
}  // namespace fl

using namespace fl;
using namespace fl::fbank;

extern "C" int fl_filterbank_supports(int K, int max_roots) {
    return K >= 1 && K <= FL_FILTERBANK_MAXK && max_roots >= 0 && max_roots <= FL_FILTERBANK_MAXP;
}

extern "C" long fl_filterbank_const_elems(int K) { return fl_filterbank_supports(K, 0) ? (long)K * BAND : -1; }

FL_ENTRY_F32_F64(fl_filterbank_fwd, (const void* X, long pitch_x, long rows, long M, const void* consts, int K, void* Y, long pitch_y,
                                     void* stream),
                 (X, pitch_x, rows, M, consts, K, Y, pitch_y, stream)) {
    FL_REQUIRE(X && consts && Y, "filterbank_fwd: null pointer");
    FL_FBANK_SIZES("filterbank_fwd");
    hipLaunchKernelGGL((fbank_fwd_kernel<T>), dim3((unsigned)cdiv_i(M, 256), (unsigned)K), dim3(256), 0, (hipStream_t)stream,
                       (const cx<T>*)X, pitch_x, rows, M, (const double*)consts, K, (cx<T>*)Y, pitch_y);
    FL_CHECK_LAUNCH("filterbank_fwd");
    return FL_OK;
}

FL_ENTRY_F32_F64(fl_filterbank_bwd, (const void* gY, long pitch_y, long rows, long M, const void* consts, int K, void* gX, long pitch_x,
                                     void* stream),
                 (gY, pitch_y, rows, M, consts, K, gX, pitch_x, stream)) {
    FL_REQUIRE(gY && consts && gX, "filterbank_bwd: null pointer");
    FL_FBANK_SIZES("filterbank_bwd");
    hipLaunchKernelGGL((fbank_bwd_kernel<T>), dim3((unsigned)cdiv_i(M, 256), (unsigned)cdiv_i(rows, RB)), dim3(256), 0,
                       (hipStream_t)stream, (const cx<T>*)gY, pitch_y, rows, M, (const double*)consts, K, (cx<T>*)gX, pitch_x);
    FL_CHECK_LAUNCH("filterbank_bwd");
    return FL_OK;
}
