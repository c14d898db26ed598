// ckl_recompress: a stream's labels re-encoded without its voxels.  After a TABLES run the decoder holds, per
// slice, the horizontal runs (word_base, run_cc: ckl_run_types.hpp) and the component -> label map; the label of
// a pixel is a function of its run.  The encoder needs the volume for three things only, and all three follow
// from (runs, label of every run):
//   k_label_planes_from_runs       the "differs from the neighbour" planes, their per-slice counts and the
//                                  row / slice wrap-arounds of lib::pixel_pairs (lib.hpp:249-256)
//   k_label_map_max                lib::max_label (lib.hpp:224-247): every component has a pixel
//   k_component_labels_from_runs   the label of every component of the NEW planes, from its first pixel
//                                  (what k_mapping_comps and k_slice_resolve_enc read from the volume)
// The first two are launched by the road itself (ckl_recompress.hip), the third by the encoder's label stage
// (flat_launch_resolve / flat_collect, ckl_encode_labels.hip): two units see this header, so its kernels are static.
#pragma once

#include "ckl_run_types.hpp"

namespace ckl {
namespace dev {

// the decoder's tables (device pointers; valid while the decode session lives)
struct RunLabels {
	RunGeom g;                      // the DECODER's crack planes: breaks() by the stream's crack format
	const uint32_t* word_base;      // [nslices][plane_words]
	const uint64_t* rbase;          // per slice base into run_cc
	const uint32_t* run_cc;         // component of every run
	const uint32_t* nruns;          // [nslices]
	const uint64_t* comp_off;       // per slice base into label_map
	const uint32_t* ncomp;          // [nslices] components as the label section states them
	const uint64_t* label_map;      // component -> label
	const uint32_t* keep = nullptr; // ckl_erode.hpp: [nslices][plane_words], a pixel whose bit is 0 carries label 0 (nullptr: every pixel keeps its label)
	// ckl_dilate.hpp: a pixel whose bit is set in gain [nslices][plane_words] carries gain_label[gain_off[its word] + the set
	// bits of the word below it] instead of its run's label (nullptr: no pixel does)
	const uint32_t* gain = nullptr;
	const uint64_t* gain_off = nullptr;
	const uint64_t* gain_label = nullptr;
	// ckl_downsample.hpp: the encoder's volume is the pooled one, of another shape than the decoder's.  pool_cut
	// [osz][pool_plane_words]: bit x set where pixel x of the word's row may change its pooled label (bit 0 of every word
	// is set); the pixel carries pool_label[pool_off[its word] + the set bits of the word at or below it - 1] (nullptr: no
	// pooling, the encoder's volume has the decoder's shape).  The triple has two producers: ckl_downsample.hpp (the pooled
	// shape) and ckl_combine.hpp (two streams merged by a rule; pool_sx .. pool_plane_words are then the decoder's own)
	const uint32_t* pool_cut = nullptr;
	const uint64_t* pool_off = nullptr;
	const uint64_t* pool_label = nullptr;
	uint32_t pool_sx = 0, pool_sy = 0, pool_row_words = 0;
	uint64_t pool_plane_words = 0;

	// the labels of one slice's runs, the slice's bases fetched once; everything read from the tables is clamped as
	// k_paint_window clamps it
	struct Slice {
		const uint32_t* rcc;
		const uint64_t* lmap;
		uint32_t n, last, nce;      // runs of the slice, its last run (0 without any), components
		__device__ __forceinline__ uint64_t operator()(uint32_t run) const {
			if (!n) return 0ull;
			const uint32_t cc = rcc[run < last ? run : last];
			return cc < nce ? lmap[cc] : 0ull;
		}
	};
	__device__ __forceinline__ Slice slice(uint32_t zi) const {
		const uint32_t n = nruns[zi];
		return { run_cc + rbase[zi], label_map + comp_off[zi], n, n ? n - 1u : 0u, ncomp[zi] };
	}
	// label of run `run` of slice zi
	__device__ __forceinline__ uint64_t label_of(uint32_t zi, uint32_t run) const { return slice(zi)(run); }
	// true, and the label in l: pixel (x, y) of slice zi is a gained one
	__device__ __forceinline__ bool gained(uint32_t zi, uint32_t x, uint32_t y, uint64_t& l) const {
		if (!gain) return false;
		const uint64_t at = zi * g.plane_words + static_cast<uint64_t>(y) * g.row_words + (x >> 5);
		const uint32_t gw = gain[at], bit = 1u << (x & 31u);
		if (!(gw & bit)) return false;
		l = gain_label[gain_off[at] + __popc(gw & (bit - 1u))];
		return true;
	}
	// the pooled label of pixel (x, y) of slice zi of the POOLED volume (pool_cut is not null)
	__device__ __forceinline__ uint64_t pooled(uint32_t zi, uint32_t x, uint32_t y) const {
		const uint64_t at = zi * pool_plane_words + static_cast<uint64_t>(y) * pool_row_words + (x >> 5);
		return pool_label[pool_off[at] + __popc(pool_cut[at] & mask_le(x & 31u)) - 1u];
	}
	// the run of pixel (x, y) of slice zi
	__device__ __forceinline__ uint32_t run_at(uint32_t zi, uint32_t x, uint32_t y) const {
		const uint32_t w = x >> 5;
		return word_base[zi * g.plane_words + static_cast<uint64_t>(y) * g.row_words + w] + __popc(g.breaks(zi, y, w) & mask_le(x & 31u)) - 1u;
	}
};

// The tail of the three plane writers (here, ckl_erode.hpp, ckl_dilate.hpp): a thread's bits of V, bits of H and wrap
// pairs, summed over the workgroup, into slice zi's entries of counts [3][nslices].  Every thread of the workgroup calls it.
__device__ __forceinline__ void add_plane_counts(uint32_t nv, uint32_t nh, uint32_t nw, uint32_t* s_red, uint32_t* counts, uint32_t nslices, uint32_t zi) {
	nv = block_sum(nv, s_red); nh = block_sum(nh, s_red); nw = block_sum(nw, s_red);
	if (threadIdx.x == 0) {
		if (nv) atomicAdd(counts + zi, nv);
		if (nh) atomicAdd(counts + nslices + zi, nh);
		if (nw) atomicAdd(counts + 2u * nslices + zi, nw);
	}
}

// One thread per 32-pixel word (zi, y, w).  The runs of a word are consecutive, word_base + k for its k-th break,
// so a thread fetches one label per run, not per pixel.
//   V: bit x (1 <= x < sx) where a run starts at x and its label differs from the run before it.
//   H (y >= 1): the word cut at breaks(y) | breaks(y - 1); inside a piece both rows have one label each, and the
//      piece's bits are set when those differ.
// Bits at or past sx, x = 0 of V and y = 0 of H stay 0, as k_label_planes leaves them: the planes are a function of
// the labels alone, whatever the input's crack format.
// counts (zeroed by the host): [nslices] bits of V, [nslices] bits of H, [nslices] wrap pairs — the first pixel of
// a row equal to the pixel before it in x-fastest order (the last of the row above, or of the slice before).
// grid = (ceil(plane_words / 256), nslices)
static __global__ void __launch_bounds__(kBlock) k_label_planes_from_runs(
	RunLabels t, uint32_t* __restrict__ planeV, uint32_t* __restrict__ planeH, uint32_t* __restrict__ counts, uint32_t nslices
) {
	__shared__ uint32_t s_red[kWaves];
	const RunGeom& g = t.g;
	const uint32_t zi = blockIdx.y;
	const uint64_t i = this_word();
	uint32_t nv = 0, nh = 0, nw = 0;
	if (i < g.plane_words) {
		const auto [y, w, valid, at] = PlaneWord(g, zi, i);
		const RunLabels::Slice label_of = t.slice(zi);
		const uint32_t b = g.breaks(zi, y, w);
		const uint32_t bu = y ? g.breaks(zi, y - 1u, w) : 0u;
		uint32_t rc = t.word_base[at] - 1u;                                // the run that reaches into the word from the left
		uint32_t ru = y ? t.word_base[at - g.row_words] - 1u : 0u;         // (w = 0: the last run of the row before)
		uint64_t lc = 0, lu = 0;
		if (w == 0) {
			// the row's first pixel against the pixel before it in linear order
			if (y) nw = label_of(rc) == label_of(rc + 1u);
			else if (zi) nw = t.label_of(zi - 1u, 0xFFFFFFFFu) == label_of(0u);
		}
		else {
			lc = label_of(rc);
			if (y && !(bu & 1u)) lu = label_of(ru);
		}
		uint32_t v = 0, h = 0;
		uint32_t rest = y ? ((b | bu | 1u) & valid) : b;
		while (rest) {
			const uint32_t x = __builtin_ctz(rest);
			rest &= rest - 1u;
			if ((b >> x) & 1u) {
				const uint64_t l = label_of(++rc);
				if ((w | x) && l != lc) v |= 1u << x;
				lc = l;
			}
			if (y) {
				if ((bu >> x) & 1u) lu = label_of(++ru);
				if (lc != lu) h |= bits_from_to(x, rest ? __builtin_ctz(rest) : 32u);      // the piece ends at the next cut
			}
		}
		h &= valid;
		planeV[at] = v; planeH[at] = h;
		nv = __popc(v); nh = __popc(h);
	}
	add_plane_counts(nv, nh, nw, s_red, counts, nslices, zi);
}

// the largest entry of the component -> label map; *out zeroed by the host
static __global__ void __launch_bounds__(kBlock) k_label_map_max(const uint64_t* __restrict__ label_map, uint64_t n, unsigned long long* __restrict__ out) {
	__shared__ unsigned long long s_max[kWaves];
	unsigned long long mx = 0;
	const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
	for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
		const unsigned long long v = label_map[i];
		mx = v > mx ? v : mx;
	}
	block_max_into(mx, s_max, out);
}

// One thread per component of the NEW planes: its first pixel (the strip path leaves it in the resolve's slots, the
// run pipeline in comp_pix) -> the decoder's run at that pixel -> its label; of a pooled volume (ckl_downsample.hpp),
// whose slices have another shape than the decoder's, the pooled run at that pixel.  ncomp / comp_off / rbase_enc are
// the ENCODER's, and so is the row length the pixel is split by.  grid = (ceil(most components of a slice / 256), nslices)
static __global__ void __launch_bounds__(kBlock) k_component_labels_from_runs(
	RunLabels t, const uint64_t* __restrict__ slots, uint32_t slot_cap, const uint32_t* __restrict__ comp_pix, const uint64_t* __restrict__ rbase_enc,
	const uint32_t* __restrict__ ncomp, const uint64_t* __restrict__ comp_off, uint64_t* __restrict__ mapping
) {
	const uint32_t zi = blockIdx.y;
	const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
	if (c >= ncomp[zi]) return;
	// the slice of the ENCODER's volume: the pooled one's (ckl_downsample.hpp), otherwise the decoder's
	const uint32_t sx = t.pool_cut ? t.pool_sx : t.g.sx, sy = t.pool_cut ? t.pool_sy : t.g.sy;
	const uint32_t n_pixels = sx * sy;
	uint32_t pix = slots ? static_cast<uint32_t>(slots[static_cast<uint64_t>(zi) * slot_cap + c]) : comp_pix[rbase_enc[zi] + c];
	pix = pix < n_pixels ? pix : n_pixels - 1u;
	const uint32_t y = pix / sx;
	const uint32_t x = pix - y * sx;
	if (t.pool_cut) { mapping[comp_off[zi] + c] = t.pooled(zi, x, y); return; }
	const bool kept = !t.keep || ((t.keep[zi * t.g.plane_words + static_cast<uint64_t>(y) * t.g.row_words + (x >> 5)] >> (x & 31u)) & 1u);
	uint64_t l;
	if (!t.gained(zi, x, y, l)) l = kept ? t.label_of(zi, t.run_at(zi, x, y)) : 0ull;
	mapping[comp_off[zi] + c] = l;
}

}  // namespace dev
}  // namespace ckl
