// zpack.cuh — the device side of compact assignments (the "ZKHIPZ1" form of include/zkhip.h; the host packer, the unpacker and
// the validation of a buffer are in ingest.hip).  One kernel widens a packed assignment into the m x 32 B canonical form the
// provers read, in place of the copy of those bytes and k_check_canonical.
//
// The host has validated the whole buffer before it is copied (assignment_packed_validate): the index is monotone, 16-aligned and
// the span of every block is the 16-rounded sum of the widths its tags name, at most 32 KiB.  The kernel relies on that and clamps
// nothing.
#pragma once
#include "devrt.h"
#include "field.cuh"

namespace zk {

static constexpr u32 ZPACK_BLOCK_ELEMS = 1024;                        // elements per block = 4 per work-item x 256
static constexpr u32 ZPACK_STAGE_BYTES = ZPACK_BLOCK_ELEMS * 32;      // a block of 32-byte values: the widest payload span

// payload bytes of width class c (0: the value 0, 1: one byte, 2: eight, 3: thirty-two)
__device__ __forceinline__ u32 zpack_width(u32 c) { return (0x20080100u >> (8 * c)) & 0xffu; }

// One workgroup of 256 = one block of 1024 elements; work-item t owns elements 4t .. 4t+3 of it, i.e. tag byte t.
//   tags, index, payload : the three sections of the packed buffer in device memory (each 16-byte aligned)
//   out                  : m x 32 B, canonical integers
//   flag                 : |= 1 if a class-3 value is >= the modulus (classes 0-2 are below 2^64)
template <class F>
__global__ void __launch_bounds__(256) k_unpack_assignment(const uint8_t* __restrict__ tags, const u64* __restrict__ index,
                                                           const uint8_t* __restrict__ payload, F* __restrict__ out, u64 m, u32* __restrict__ flag) {
    static_assert(F::N == 8, "a scalar field of eight 32-bit words");
    ZK_PRIO_HIGH();
    // the block's payload span, and one slot more: a value's words are picked out of pairs of aligned words, and the pair of the
    // last word of a full span ends one word past it
    __shared__ uint4 stage[ZPACK_STAGE_BYTES / 16 + 1];
    __shared__ u32 wave_sum[4];
    const u32 t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const u64 blk = blockIdx.x;
    const u64 e0 = blk * ZPACK_BLOCK_ELEMS + 4 * (u64)t;
    const u32 tg = e0 < m ? tags[blk * (ZPACK_BLOCK_ELEMS / 4) + t] : 0;      // (tag byte i exists iff element 4i does)
    const u32 bytes = zpack_width(tg & 3) + zpack_width((tg >> 2) & 3) + zpack_width((tg >> 4) & 3) + zpack_width(tg >> 6);
    // inclusive scan of the byte counts over the wave
    u32 incl = bytes;
    ZK_UNROLL for (u32 d = 1; d < 64; d <<= 1) {
        const u32 up = __shfl(incl, (int)(lane >= d ? lane - d : lane));
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    // stage the span: 16-byte loads, consecutive work-items consecutive slots
    const u64 p0 = index[blk];
    const u32 n16 = (u32)((index[blk + 1] - p0) >> 4);
    const uint4* __restrict__ src = (const uint4*)(payload + p0);
    for (u32 i = t; i < n16; i += 256) stage[i] = src[i];
    __syncthreads();
    u32 off = incl - bytes;
    ZK_UNROLL for (u32 k = 0; k < 3; ++k)
        if (k < wave) off += wave_sum[k];
    const u32* __restrict__ words = (const u32*)stage;
    uint4* __restrict__ dst = (uint4*)(out + e0);
    bool too_big = false;
    ZK_UNROLL for (u32 j = 0; j < 4; ++j) {
        const u32 c = (tg >> (2 * j)) & 3;
        // the aligned words that hold the value (2 for one byte, 3 for eight, 9 for thirty-two: it may start at any byte), then
        // each of its words from two neighbours
        const u32 base = off >> 2, sh = 8 * (off & 3);
        const u32 nread = c == 3 ? 9 : c == 2 ? 3 : c == 1 ? 2 : 0;
        u32 a[9];
        ZK_UNROLL for (u32 k = 0; k < 9; ++k) a[k] = k < nread ? words[base + k] : 0;
        u32 v[8];
        ZK_UNROLL for (u32 k = 0; k < 8; ++k) v[k] = (u32)((((u64)a[k + 1] << 32) | a[k]) >> sh);
        if (c == 1) v[0] &= 0xffu;
        const u32 nw = c == 3 ? 8 : c == 2 ? 2 : c;      // words of the value; the rest is zero
        ZK_UNROLL for (u32 k = 1; k < 8; ++k)
            if (k >= nw) v[k] = 0;
        if (c == 0) v[0] = 0;
        if (c == 3) {
            bool lt = false, decided = false;
            ZK_UNROLL for (int k = F::N - 1; k >= 0; --k) {
                if (!decided && v[k] != F::Params::mod(k)) { lt = v[k] < F::Params::mod(k); decided = true; }
            }
            too_big = too_big || !lt;
        }
        if (e0 + j < m) {      // (the last block: elements past m are not written)
            dst[2 * j] = make_uint4(v[0], v[1], v[2], v[3]);
            dst[2 * j + 1] = make_uint4(v[4], v[5], v[6], v[7]);
        }
        off += zpack_width(c);
    }
    if (too_big) atomicOr(flag, 1u);
}

}  // namespace zk
