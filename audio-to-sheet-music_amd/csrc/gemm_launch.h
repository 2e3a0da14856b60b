// Host side shared by the GEMM kernel families (internal: gemm*.hip, rowln.hip, tools/): the families' entry points,
// the resident-block cache, the epilogue-form dispatch and the profile scope of a launch.
#pragma once
#include "common.h"
#include "prof.h"
#include "gemm.h"
#include "gemm_epi.h"

#include <type_traits>

namespace athd {

// Entry points of the kernel families gemm_launch routes to (gemm.h: gemm_route).  *_supported: the shapes a family
// handles; *_launch: hipGetLastError(), or -2 for a descriptor that is not the family's.
bool gemm2_supported(const GemmDesc& d);
int gemm2_launch(const GemmDesc& d, hipStream_t s);
bool gemm3_supported(const GemmDesc& d);
// route: ROUTE_GEMM3_V3 (256 x 192 tiles, 2 stages) or ROUTE_GEMM3_V7 (192 x 192, 3 stages), both persistent
int gemm3_launch(const GemmDesc& d, hipStream_t s, GemmRoute route);
bool gemm3_ln_supported(const GemmDesc& d);
int gemm3_ln_launch(const GemmDesc& d, hipStream_t s);
bool gemm5_supported(const GemmDesc& d);
int gemm5_launch(const GemmDesc& d, hipStream_t s);
int rowln_launch(const GemmDesc& d, hipStream_t s);
bool rowln_text_enabled();
bool rowln_text_supported(const GemmDesc& d);
int rowln_text_launch(const GemmDesc& d, hipStream_t s);
#ifdef ATHD_KBENCH   // tools/libkbench.so only
int gemm3_variant_launch(const GemmDesc& d, hipStream_t s, int variant);   // gemm3.hip: the tile-shape table
int gemm4_launch(const GemmDesc& d, hipStream_t s);
int gemm5_probe_launch(const GemmDesc& d, hipStream_t s, int probe);
int gemm6_launch(const GemmDesc& d, hipStream_t s);
#endif

// Blocks of Kernel resident on the current device at `threads` per block: per CU from the occupancy API, asked once
// per kernel (a property of the kernel), times the current device's CU count.  0: unknown.
template <auto Kernel>
int64_t resident_blocks(int threads) {
    static int per_cu = 0;
    if (per_cu == 0) {
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, threads, 0);
        if (per_cu <= 0) per_cu = -1;
    }
    return per_cu > 0 ? (int64_t)per_cu * device_cus() : 0;
}

// f(std::integral_constant<unsigned, F>) for the epilogue form F of `flags`: one of ATHD_EPI_LIST, else F_ALL
template <typename Fn>
void dispatch_epi(unsigned flags, Fn&& f) {
    switch (flags) {
#define ATHD_CASE(FL) \
    case (FL): f(std::integral_constant<unsigned, (FL)>{}); return;
        ATHD_EPI_LIST(ATHD_CASE)
#undef ATHD_CASE
        default: f(std::integral_constant<unsigned, F_ALL>{}); return;
    }
}

// Profile scope of one GEMM launch (prof.h): label = the kernel's symbol as klabel(fmt, ...) prints it, work =
// gemm_work(d, mode).  Lives until the kernel is launched.
struct GemmScope : KScope {
    template <typename... Args>
    GemmScope(hipStream_t s, const GemmDesc& d, int mode, const char* fmt, Args... args) : KScope(s) {
        if (!on()) return;
        double fl, by;
        gemm_work(d, mode, fl, by);
        begin(klabel(fmt, args...), fl, by);
    }
};

}  // namespace athd
