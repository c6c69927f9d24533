// How a volume-augmentation launch is cut, kept once for biu_augment_vol.hip (batches of stored tiles) and biu_augment_vol_crop.hip (crops
// out of whole volumes): both launches are planned from the shape of what they WRITE, so biu_augment_vol_chunk answers for both.
#pragma once
#include "biu_common.h"

namespace biu_augment_vol_plan {
constexpr int TPB = 256;
constexpr int TILE = 64;                        // the tile kernel's output tile is TILE x TILE
constexpr int MAX_CHUNK = 16;                   // planes a lane walks with one set of taps, at most

// Planes per lane (per block of the tile kernel): as many as MAX_CHUNK, halved while the launch would have fewer than 2048 blocks, 8 for
// each of the 256 compute units.  That figure is a guess at what hides the tail of the last wave of blocks; it has not been measured
// against other values.
struct Plan {
    bool tile, rows;
    int units, tx, ty, chunk, nchunks;
};
inline Plan plan_of(int n, int channels, int depth, int h, int w, int kind, int max_blur_k, bool aligned16) {
    Plan p;
    p.tile = kind == BIU_AUGF_IMAGE && max_blur_k > 1;
    p.rows = w % 4 == 0 && aligned16;
    p.units = kind == BIU_AUGF_VECTOR ? channels / 2 * depth : channels * depth;
    p.tx = (w + TILE - 1) / TILE;
    p.ty = (h + TILE - 1) / TILE;
    const i64 work = p.tile ? (i64)n * p.tx * p.ty : (i64)n * (p.rows ? h * (w / 4) : h * w);      // blocks, or lanes, per chunk
    const i64 want = p.tile ? 2048 : (i64)2048 * TPB;
    int c = MAX_CHUNK;
    while (c > 1 && work * ((p.units + c - 1) / c) < want) c >>= 1;
    p.chunk = p.units < c ? p.units : c;
    p.nchunks = (p.units + p.chunk - 1) / p.chunk;
    return p;
}
}  // namespace biu_augment_vol_plan
