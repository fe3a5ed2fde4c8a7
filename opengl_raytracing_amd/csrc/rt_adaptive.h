// rt_adaptive.h -- adaptive sampling's launch wrappers: what rt_adaptive.hip implements for the entry points in rt_adaptive.cpp
// (rt_accum_select, rt_accum_add_at; include/rt_mi355.h has the definition).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rt_accum.h"

// The selection's geometry: tiles of 8 x 8 pixels (one wave each), chunks of 32 consecutive tiles (one workgroup's step), and at
// most kSelectMaxWgs workgroups, each owning a contiguous run of chunks -- so one workgroup scans all their totals in one pass.
constexpr unsigned kSelectTile = 8, kSelectTilesPerChunk = 32, kSelectMaxWgs = 512;
constexpr size_t kSelectScratchHeader = 2 * kSelectMaxWgs * sizeof(uint32_t);   // the workgroups' selected and capped totals

inline uint64_t rt_select_tiles(int width, int height) {
    return (((uint64_t)width + kSelectTile - 1) / kSelectTile) * (((uint64_t)height + kSelectTile - 1) / kSelectTile);   // width up to 2^31 - 1
}
// header + one 64-bit ballot per tile (a multiple of 16 bytes)
inline size_t rt_select_scratch_bytes(int width, int height) {
    return kSelectScratchHeader + (((size_t)rt_select_tiles(width, height) * 8 + 15) & ~(size_t)15);
}

// The grid every kernel of the selection is launched with, for a width x height image (width * height <= 2^31 - 1)
struct RtSelectGrid {
    unsigned tilesX, nTiles, nChunks, chunksPerWg, nWgs;
    RtSelectGrid(int width, int height) {
        tilesX = ((unsigned)width + kSelectTile - 1u) / kSelectTile;
        nTiles = (unsigned)rt_select_tiles(width, height);
        nChunks = (nTiles + kSelectTilesPerChunk - 1u) / kSelectTilesPerChunk;
        chunksPerWg = (nChunks + kSelectMaxWgs - 1u) / kSelectMaxWgs;
        nWgs = (nChunks + chunksPerWg - 1u) / chunksPerWg;                          // <= kSelectMaxWgs, none without a chunk
    }
};

// The selection's second half, for any kernel that left one ballot per tile and the two totals of every workgroup of RtSelectGrid
// in scratch (the judge below; rt_upsample.hip's reconstruction): scan (offsets, the select state), emit (the list) -- two launches
// on s; the emit is left out when capacity == 0.
hipError_t rt_launch_select_from_ballots(void *scratch, int width, int height, void *pixels, unsigned capacity, void *selState, hipStream_t s);
// rt_accum_select: judge (ballots and the workgroups' totals into scratch), then rt_launch_select_from_ballots --
// three launches on s; the emit is left out when capacity == 0.  capacity <= 2^32 - 1 (the caller saturates it).
hipError_t rt_launch_accum_select(const void *accum, int width, int height, const RtAccumRule &rule, unsigned maxSamples, void *pixels,
                                  unsigned capacity, void *scratch, void *selState, hipStream_t s);
// rt_accum_add_at: clear of the state except `frames`, scatter (left out when n == 0), statistics over every pixel, solve.
// n is at most one grid of 256-lane workgroups (callers refuse more first)
hipError_t rt_launch_accum_add_at(const void *samples, const void *pixels, size_t n, void *accum, void *state, int width, int height,
                                  const RtAccumRule &rule, hipStream_t s);
