// The XCD tile walk of the MFMA kernels.  Depends on nothing: a host compiler can include it (tools/tile_walk_hostcheck.cpp).
#pragma once

// Block -> tile, a bijection of 0..n_tiles-1 for a grid of n_tiles blocks.  The hardware deals consecutive block ids round-robin
// over the 8 XCDs; here each XCD (block % 8) walks a contiguous run of tiles, so neighbouring tiles share its L2.  The first
// n_tiles % 8 XCDs get one tile more; with n_tiles < 8 the XCDs from n_tiles on get none.
#ifdef __HIPCC__
__host__ __device__
#endif
constexpr int sq_xcd_tile(int block, int n_tiles) {
    const int q = n_tiles >> 3, r = n_tiles & 7, xcd = block & 7, idx = block >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
