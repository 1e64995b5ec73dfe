// search_scan.h — the launch path of the streaming top-k scans of the exact index, once: search_scan_kernel (k_search.hip) and
// group_scan_kernel (k_group.hip) are launched through launch_scan<Family>: the kernel per stored dtype x QT x MASKED x the scan's flag
// (SELF / OWN), the LDS size from the scan's array count, the opt-in past 64 KB.  A family names the scan:
//   typedef ... Params;   static constexpr int ARRAYS;   template <typename T, int QT, bool MASKED, bool FLAG> static auto kernel();
//   static bool flag(const Params &);   static Params params(const ScanArgs &);
// The two kernels keep their own texts and parameter structs.  One shared body (a function template over a selection policy and one
// struct for both) was built and measured: it compiled to 0 ... +7 / -2 ... +4 instructions per kernel in another order, and the masked
// i8 scan and the scan over small indexes came out 4-5 % slower (profiles/scan_engine_refactor.txt).
// LDS per workgroup: scan_lds_bytes = 2 * 16 QT * 4 (counts, thresholds) + 4 waves * ARRAYS * P * 4, P = search_sort_size(k) <= 2048.
#pragma once

#include "search_common.h"

namespace clipamd {

// the grouped half of launch_search_scan (k_group.hip: a.groups != NULL)
bool launch_group_scan(const ScanArgs & a, hipStream_t stream);

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int ROWS_PER_ITER = 64;     // 4 waves x 16 rows

constexpr size_t scan_lds_bytes(int qt, int arrays, int P) { return (size_t)2 * 16 * qt * 4 + (size_t)4 * arrays * P * 4; }

template <typename Family, typename T, int QT, bool MASKED, bool FLAG>
bool launch_scan_m(const typename Family::Params & p, int n_chunks, hipStream_t stream) {
    static unsigned long long lds_done = 0;
    const auto kernel = Family::template kernel<T, QT, MASKED, FLAG>();
    const size_t lds = scan_lds_bytes(QT, Family::ARRAYS, p.P);
    if (lds > 65536) opt_in_dynamic_lds(kernel, lds, lds_done);
    const dim3 grid(n_chunks, (p.nq + 16 * QT - 1) / (16 * QT));
    hipLaunchKernelGGL(kernel, grid, dim3(SCAN_THREADS), lds, stream, p);
    return hipGetLastError() == hipSuccess;
}

template <typename Family, typename T, int QT>
bool launch_scan_t(const typename Family::Params & p, int n_chunks, hipStream_t stream) {
    if (Family::flag(p))
        return p.mask ? launch_scan_m<Family, T, QT, true, true>(p, n_chunks, stream)
                      : launch_scan_m<Family, T, QT, false, true>(p, n_chunks, stream);
    return p.mask ? launch_scan_m<Family, T, QT, true, false>(p, n_chunks, stream) : launch_scan_m<Family, T, QT, false, false>(p, n_chunks, stream);
}

template <typename Family>
bool launch_scan(const ScanArgs & a, hipStream_t stream) {
    const typename Family::Params p = Family::params(a);
    return with_search_type(a.dtype, [&](auto t) {
        using T = decltype(t);
        if (a.qt == 4) return launch_scan_t<Family, T, 4>(p, a.n_chunks, stream);
        if (a.qt == 2) return launch_scan_t<Family, T, 2>(p, a.n_chunks, stream);
        return launch_scan_t<Family, T, 1>(p, a.n_chunks, stream);
    });
}

}  // namespace

}  // namespace clipamd
