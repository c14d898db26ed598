// The crack planes and run tables as the kernels see them, and the slices' error bits: what the
// run kernels (ckl_runs.hpp) build and what everything that reads their tables needs.
#pragma once

#include "ckl_device.hpp"

namespace ckl {
namespace dev {

enum : uint32_t {
	ERR_BOC = 1u,          // beginning-of-chain index malformed
	ERR_RANGE = 2u,        // a move left the vertex grid
	ERR_CAPACITY = 4u,     // scratch capacity exceeded
	ERR_NCOMP = 8u,        // component count differs from the label section
	ERR_CRC = 16u,         // crc32c of the component image differs from the stored one
	ERR_LIST = 32u,        // a strip's record list overflowed (k_crack_records): not an error of the stream, the rasterising path takes over
};

// ------------------------------------------------------------------------------
// horizontal runs
// ------------------------------------------------------------------------------
// A run is a maximal stretch of horizontally connected pixels of one row.  Runs are
// numbered in raster order of their first pixel; word_base[w] = number of runs that
// start before 32-pixel word w of the slice, so the run of pixel (x, y) is
//   word_base[y, x>>5] + popcount(breaks(y, x>>5) & bits <= (x & 31)) - 1.
struct RunGeom {
	const uint32_t* planeV;
	const uint32_t* planeH;
	uint32_t row_words;
	uint64_t plane_words;
	uint32_t flip;          // 1 for IMPERMISSIBLE (a crack bit is a break)
	uint32_t sx, sy;
	__device__ __forceinline__ uint32_t valid_mask(uint32_t w) const {
		const uint32_t left = sx - w * 32u;
		return left >= 32u ? 0xFFFFFFFFu : ((1u << left) - 1u);
	}
	// bit x set: a run starts at pixel x of this word
	__device__ __forceinline__ uint32_t breaks(uint32_t zi, uint32_t y, uint32_t w) const {
		const uint32_t v = planeV[zi * plane_words + static_cast<uint64_t>(y) * row_words + w];
		uint32_t b = flip ? v : ~v;
		if (w == 0) b |= 1u;
		return b & valid_mask(w);
	}
	// bit x set: pixel x is connected to the pixel above it
	__device__ __forceinline__ uint32_t ups(uint32_t zi, uint32_t y, uint32_t w) const {
		if (y == 0) return 0u;
		const uint32_t h = planeH[zi * plane_words + static_cast<uint64_t>(y) * row_words + w];
		return (flip ? ~h : h) & valid_mask(w);
	}
	// the same from a plane word that is already loaded (the strip kernels issue all their loads
	// first, unconditionally, and interpret the words afterwards: a load inside a branch is
	// waited for inside the branch)
	__device__ __forceinline__ uint32_t breaks_of(uint32_t v, uint32_t w) const {
		uint32_t b = flip ? v : ~v;
		if (w == 0) b |= 1u;
		return b & valid_mask(w);
	}
	__device__ __forceinline__ uint32_t ups_of(uint32_t h, uint32_t w) const { return (flip ? ~h : h) & valid_mask(w); }
};
__device__ __forceinline__ uint32_t mask_le(uint32_t bit) { return bit >= 31u ? 0xFFFFFFFFu : ((2u << bit) - 1u); }
// bits [x, end) of a word
__device__ __forceinline__ uint32_t bits_from_to(uint32_t x, uint32_t end) {
	return (end >= 32u ? 0xFFFFFFFFu : ((1u << end) - 1u)) & ~((1u << x) - 1u);
}

// The 32-pixel word i (< plane_words) of slice zi: its row, its place in the row, its index in an [nslices][plane_words]
// array and its pixels inside the row.  this_word(): the word of a thread in a grid of (ceil(plane_words / 256), nslices).
__device__ __forceinline__ uint64_t this_word() { return static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; }
struct PlaneWord {
	uint32_t y, w, valid;
	uint64_t at;
	__device__ __forceinline__ PlaneWord(const RunGeom& g, uint32_t zi, uint64_t i)
		: y(static_cast<uint32_t>(i / g.row_words)), w(static_cast<uint32_t>(i - static_cast<uint64_t>(y) * g.row_words)), valid(g.valid_mask(w)), at(zi * g.plane_words + i) {}
};

struct RunArrays {
	uint32_t* word_base;       // [nslices][plane_words]
	const uint64_t* rbase;     // per slice base into the run arrays
	const uint32_t* rcap;
	uint32_t* parent;          // union-find over runs (root = smallest run index)
	uint32_t* run_start;       // first pixel of the run (slice-linear)
	uint32_t* run_cc;          // component id of the run
	uint32_t* comp_pix = nullptr;      // optional, [at rbase, one entry per component]: first pixel of the component (its root run's start)
	uint32_t* nruns;           // [nslices]
	uint32_t* ncomp;           // [nslices]
	uint32_t* slice_err;
};

}  // namespace dev
}  // namespace ckl
