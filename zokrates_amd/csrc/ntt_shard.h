// Geometry of a transform whose domain is sharded across the members of a zkhip_multi: ONE definition, plain
// C++ (no device code), the same on every member and in tests/host/ntt_shard_layout.cpp.
//
// A plan's domain N = N1 x Nb (Nb = N2 * N3) is a row-major N1 x Nb matrix, G the number of members:
//   strip  S_k   columns [k Nb/G, (k+1) Nb/G) of every row: member k runs the outer cols pass (over N1) on it
//   range  R_k   elements [k N/G, (k+1) N/G) = outer indices [k N1/G, (k+1) N1/G) as whole blocks of Nb: everything after the
//                outer pass (rows; mid and rows of three passes)
//   block (r, c) rows of R_r x columns of S_c: N1/G rows of Nb/G contiguous elements, Nb apart
// Between the two an all-to-all moves every block (r, c), r != c, once: natural -> sigma (kind A) from member c to member r,
// sigma -> natural (kind B) from member r to member c.  A block keeps its position in the full-length vector of its receiver.
// Every pass is the plan's kernel over a strip or a range (ntt_geom.h: ntt_pass_shape).  The whole domain is the span G = 1: one
// strip of all Nb columns, one range of all N1 outer indices, origins 0, nothing to exchange — what a single context runs.
#pragma once
#include <cstddef>
#include <cstdint>

namespace zk {

struct ShardGeom {
    uint32_t G = 0;        // members
    uint64_t N = 0, Nb = 0;
    uint32_t N1 = 0;
    uint32_t W = 0;        // strip width: Nb / G columns
    uint32_t rows = 0;     // outer indices per range: N1 / G
    uint64_t block = 0;    // elements of one block: rows * W
    // first element of strip k / range k / block (r, c) in the vector
    uint64_t strip_origin(uint32_t k) const { return (uint64_t)k * W; }
    uint64_t range_origin(uint32_t k) const { return (uint64_t)k * rows * Nb; }
    uint64_t range_len() const { return (uint64_t)rows * Nb; }
    uint64_t block_origin(uint32_t r, uint32_t c) const { return (uint64_t)r * rows * Nb + (uint64_t)c * W; }
    // staging of `nvec` vectors: slot (v, peer) holds the block exchanged with `peer` (the member's own slot stays unused in
    // an exchange; the upload of a strip fills all G), rows back to back
    uint64_t slot_origin(uint32_t v, uint32_t peer) const { return ((uint64_t)v * G + peer) * block; }
    uint64_t staging_len(uint32_t nvec) const { return (uint64_t)nvec * G * block; }
};

// G a power of two >= 2, at least two passes, a whole outer index per member, at least two columns per strip
inline bool ntt_shardable(int log1, uint32_t N1, uint64_t Nb, uint64_t G) {
    return G >= 2 && (G & (G - 1)) == 0 && log1 > 0 && G <= N1 && 2 * G <= Nb;
}
// (for a shardable transform, or G = 1: the whole domain as one span)
inline ShardGeom ntt_shard_geom(uint32_t N1, uint64_t Nb, uint32_t G) {
    ShardGeom g;
    g.G = G;
    g.N1 = N1;
    g.Nb = Nb;
    g.N = (uint64_t)N1 * Nb;
    g.W = (uint32_t)(Nb / G);
    g.rows = N1 / G;
    g.block = (uint64_t)g.rows * g.W;
    return g;
}

}  // namespace zk
