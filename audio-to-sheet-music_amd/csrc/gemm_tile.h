// Device plumbing shared by the LDS-staged bf16 GEMM kernels (gemm2 / gemm3 / gemm5 / gemm6 / rowln, tools/gemm4; the
// zero page and the fragment type also convt4): the swizzled LDS image, its LDS-DMA fill, the zero page and the counted
// wait.  The K-loops themselves (row decomposition, stages, waits, barriers) stay with each kernel: hipcc's code for
// them changes with the slightest restructuring, so they are shared only where the machine code stays the same.
//
// LDS image of one operand tile: [rows][64 bf16] = 128 B per row (LDS_ROWB), eight 16-B chunks stored XOR-swizzled
// (slot = chunk ^ (row & 7)) so that the 16x16x32 fragment reads (16 rows x one chunk per lane group) are
// conflict-free for ds_read_b128.  A wave instruction fills 8 rows x 128 B = 1 KiB; lane L lands at base + 16 L,
// i.e. row L/8, slot L%8, so it fetches global chunk (L%8) ^ (L/8): the swizzle lives in the per-lane SOURCE address
// (the LDS-DMA destination is lane-linear).  swz_chunk is that source chunk, swz_slot the byte offset a fragment
// read takes within its row.
#pragma once
#include "common.h"

namespace athd {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16v8;
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) void gbl_void;

constexpr int LDS_ROWB = 128;      // bytes per LDS row (64 bf16)

// 64 bytes of zeros: the source of out-of-range taps / rows / k.  The library is built without relocatable device
// code, so every translation unit that includes this header gets its own copy.
static __device__ __attribute__((aligned(64))) uint4 g_zero_page[4];

template <int N>
ATHD_DEV void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// global_load_lds_dwordx4: 16 B per lane from src straight into LDS at lds_dst + 16 * lane
ATHD_DEV void dma16(const void* src, void* lds_dst) {
    __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)lds_dst, 16, 0, 0);
}

ATHD_DEV int swz_chunk(int lane) { return (lane & 7) ^ (lane >> 3); }
// K sub-step ks (32 wide) of a K-tile, lane group g = lane >> 4, fragment row fr = lane & 15
ATHD_DEV int swz_slot(int ks, int g, int fr) { return ((4 * ks + g) ^ (fr & 7)) * 16; }

}  // namespace athd
