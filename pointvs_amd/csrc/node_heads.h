// The LDS tile of the per-node heads (node_heads.hip: pvs_node_heads_fwd): one lane per row, the rows `stride` floats
// apart. No HIP header: the host compiler builds this file alone (tests/test_cam_host.py reads the strides from it).
//   16-byte path (width % 4 == 0): a lane reads its row with ds_read_b128, which the LDS serves in groups of 16 lanes
//     over 64 banks; the 16 lanes of a group differ in their row number modulo 16, so their words 4 q + lane * stride
//     cover the 64 banks once when stride / 4 is odd: width, or width + 4 (68 floats at width 64, 36 at 32).
//   4-byte path (any other width): ds_read_b32 is served in groups of 32 lanes over 32 banks; an odd stride gives
//     the 32 consecutive rows of a group 32 different banks.
#pragma once

enum { kPvsNodeHeadThreads = 128, kPvsNodeHeadMaxWidth = 1024, kPvsNodeHeadTileBytes = 40960 };

inline int pvs_node_heads_stride(int width, bool vec) {
    if (!vec) return width | 1;
    return ((width >> 2) & 1) ? width : width + 4;
}

// Rows of a tile: the largest power of two, at most one per thread, whose rows fit kPvsNodeHeadTileBytes of LDS
// (128 rows up to width 76, 64 at 128, 8 at 1,024).
inline int pvs_node_heads_tile_rows(int stride) {
    int rows = kPvsNodeHeadThreads;
    while (rows > 1 && (long long)rows * stride * 4 > kPvsNodeHeadTileBytes) rows >>= 1;
    return rows;
}
