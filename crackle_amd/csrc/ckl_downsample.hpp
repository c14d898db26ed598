// ckl_downsample: the labels of a stream pooled 2 x 2 x 1 or 2 x 2 x 2, without its voxels.  The pooled volume has
// another shape than the decoder's, (ceil(sx / 2), ceil(sy / 2), ceil(sz / fz)): this is the one unit of the road whose
// word grid is the OUTPUT's (PoolGeom), while everything it reads from the decode session is the input's (RunLabels::g).
//
// The rules (label 0 is an ordinary label in both):
//   fz = 1   the reference's (src/operations.hpp:1254-1293): with a, b, c, d at (x, y), (x + 1, y), (x, y + 1),
//            (x + 1, y + 1): a == b -> a, a == c -> a, b == c -> b, else d.  A block cut by an odd sx or sy: a.
//   fz = 2   the label that occurs most often among the block's voxels that exist (8, or 4, 2, 1 at odd ends); among
//            labels tied for most often the SMALLEST, compared as unsigned 64-bit values (ckl_dilate's tie rule).  At an
//            odd sz the last output slice pools 2 x 2 x 1 blocks by THIS rule, not by the reference's.
//
// The pooled label of an output row can change only at an output pixel whose two input columns hold a break in one of
// the 2 * fz input rows under it, and at the pixel behind one whose SECOND column holds a break (its block lies in the
// new runs alone, the block before it straddles the break); everywhere else it is carried over.  So the pooled labels
// exist as runs only:
//   cut        [osz][plane_words]  bit x set: one of the input rows has a break in column 2x - 1, 2x or 2x + 1; bit 0 of
//                                  every word is set as well, so a word's labels never depend on the word before it
//   cut_off    [osz][plane_words]  where the word's cuts stand in pool_label (64-bit)
//   pool_label [cuts]              the pooled label from each cut up to the next one
// A cut is where the label MAY change: neighbouring entries can be equal.  The kernels, in launch order:
//   k_erode_run_labels   (ckl_erode.hpp) one label per input run
//   k_pool_cuts          cut from the break words of the 2 * fz input rows, two input words per output word, ORed and
//                        folded pairwise; cut_off by a scan inside the workgroup on top of a base taken from one 64-bit
//                        cursor, as k_dilate_gain takes it (the order of the bases differs from call to call; pool_label
//                        is only ever read through cut_off)
//   -- the cursor's final value, the number of cuts, crosses to the host, which sizes pool_label --
//   k_pool_labels        a thread per output word walks its cuts with one run cursor per input row: a row's label is
//                        fetched once per run, at the run's break; the rule is evaluated at each cut; the largest pooled
//                        label is taken as k_erode_keep takes the largest survivor
//   k_pool_planes        the encoder's V and H planes of the pooled labels, their per-slice counts, the wrap-around pairs,
//                        as k_label_planes_from_runs derives them from the decoder's runs
// The label stage then reads the triple through RunLabels::pooled (k_component_labels_from_runs).
#pragma once

#include "ckl_erode.hpp"

namespace ckl {
namespace dev {

// the pooled volume's word grid, beside the input's RunGeom
struct PoolGeom {
	uint32_t fz;                // 1 or 2
	uint32_t nslices_in;        // the decoder's slices
	uint32_t sx, sy;            // of the pooled volume
	uint32_t row_words;
	uint64_t plane_words;
	__device__ __forceinline__ uint32_t valid_mask(uint32_t w) const {
		const uint32_t left = sx - w * 32u;
		return left >= 32u ? 0xFFFFFFFFu : ((1u << left) - 1u);
	}
};

// the breaks of input row (z, y) in the 64 columns under output word wo: input words 2 wo (which exists where the
// output word does) and 2 wo + 1 (which may not)
__device__ __forceinline__ uint64_t pool_breaks(const RunGeom& g, uint32_t z, uint32_t y, uint32_t wo) {
	const uint32_t w0 = 2u * wo;
	uint64_t b = g.breaks(z, y, w0);
	if (w0 + 1u < g.row_words) b |= static_cast<uint64_t>(g.breaks(z, y, w0 + 1u)) << 32;
	return b;
}

// bit x of the result: bit 2x or bit 2x + 1 of b is set
__device__ __forceinline__ uint32_t pool_fold(uint64_t b) {
	uint64_t v = (b | (b >> 1)) & 0x5555555555555555ull;
	v = (v | (v >> 1)) & 0x3333333333333333ull;
	v = (v | (v >> 2)) & 0x0F0F0F0F0F0F0F0Full;
	v = (v | (v >> 4)) & 0x00FF00FF00FF00FFull;
	v = (v | (v >> 8)) & 0x0000FFFF0000FFFFull;
	return static_cast<uint32_t>(v | (v >> 16));
}

// One thread per OUTPUT word: cut and cut_off (header comment).  *cursor zeroed by the host; afterwards it holds the
// number of cuts.  No thread leaves early: the scan is the workgroup's.  grid = (ceil(p.plane_words / 256), osz)
__global__ void __launch_bounds__(kBlock) k_pool_cuts(
	RunGeom g, PoolGeom p, uint32_t* __restrict__ cut, uint64_t* __restrict__ cut_off, unsigned long long* __restrict__ cursor
) {
	__shared__ uint32_t s_scan[kWaves];
	__shared__ unsigned long long s_base;
	const uint32_t zo = blockIdx.y;
	const uint64_t i = this_word();
	const bool live = i < p.plane_words;
	const uint64_t at = zo * p.plane_words + i;
	uint32_t c = 0;
	if (live) {
		const uint32_t yo = static_cast<uint32_t>(i / p.row_words), wo = static_cast<uint32_t>(i - static_cast<uint64_t>(yo) * p.row_words);
		uint64_t b = 0;
		for (uint32_t dz = 0; dz < p.fz; dz++) {
			for (uint32_t dy = 0; dy < 2u; dy++) {
				const uint32_t z = p.fz * zo + dz, y = 2u * yo + dy;
				if (z < p.nslices_in && y < g.sy) b |= pool_breaks(g, z, y, wo);
			}
		}
		c = (pool_fold(b) | (pool_fold(b & 0xAAAAAAAAAAAAAAAAull) << 1) | 1u) & p.valid_mask(wo);      // (a break in column 63 cuts at bit 0 of the next word, which is set anyway)
		cut[at] = c;
	}
	uint32_t v[1] = { static_cast<uint32_t>(__popc(c)) }, total[1];
	block_excl_add<1>(v, total, s_scan);
	if (threadIdx.x == 0) s_base = total[0] ? atomicAdd(cursor, static_cast<unsigned long long>(total[0])) : 0ull;
	__syncthreads();
	if (live) cut_off[at] = s_base + v[0];
}

// one input row under an output word: its breaks in the word's 64 input columns, its run cursor and the label of the
// run the cursor stands on.  Every run index is clamped to the slice's runs, as SliceRunLabels clamps.
struct PoolRow {
	uint64_t b = 0, carry = 0;
	const uint64_t* lab = nullptr;
	uint32_t n = 0, run = 0;
	bool on = false;              // the row exists
	__device__ __forceinline__ uint64_t fetch(uint32_t r) const { return n ? lab[r < n ? r : n - 1u] : 0ull; }
	__device__ __forceinline__ void open(const RunLabels& t, const uint64_t* run_label, uint32_t z, uint32_t y, uint32_t wo) {
		const RunGeom& g = t.g;
		on = true;
		b = pool_breaks(g, z, y, wo);
		run = t.word_base[z * g.plane_words + static_cast<uint64_t>(y) * g.row_words + 2u * wo] - 1u;      // the run that reaches into the word from the left
		lab = run_label + t.rbase[z];
		n = t.nruns[z];
		if (!(b & 1ull)) carry = fetch(run);      // (wo = 0 has bit 0 set)
	}
	// the labels of input columns 2j and 2j + 1 of the word; called with ascending j, at every j where b has a bit (and
	// wherever else: without a bit both are the label carried over)
	__device__ __forceinline__ void pair(uint32_t j, uint64_t& first, uint64_t& second) {
		if ((b >> (2u * j)) & 1ull) carry = fetch(++run);
		first = carry;
		if ((b >> (2u * j + 1u)) & 1ull) carry = fetch(++run);
		second = carry;
	}
};

// One thread per OUTPUT word: the pooled label at each of its cuts -> pool_label, and the largest of them (one atomicMax
// per workgroup; *max_out zeroed by the host).  FZ = 1: the reference's rule; FZ = 2: the mode, ties to the smallest.
// grid = (ceil(p.plane_words / 256), osz)
template <int FZ>
__global__ void __launch_bounds__(kBlock) k_pool_labels(
	RunLabels t, const uint64_t* __restrict__ run_label, PoolGeom p, const uint32_t* __restrict__ cut, const uint64_t* __restrict__ cut_off,
	uint64_t* __restrict__ pool_label, unsigned long long* __restrict__ max_out
) {
	__shared__ unsigned long long s_max[kWaves];
	constexpr int kRows = 2 * FZ;
	const RunGeom& g = t.g;
	const uint32_t zo = blockIdx.y;
	const uint64_t i = this_word();
	unsigned long long mx = 0;
	if (i < p.plane_words) {
		const uint32_t yo = static_cast<uint32_t>(i / p.row_words), wo = static_cast<uint32_t>(i - static_cast<uint64_t>(yo) * p.row_words);
		const uint64_t at = zo * p.plane_words + i;
		PoolRow row[kRows];      // 2 * dz + dy
#pragma unroll
		for (int k = 0; k < kRows; k++) {
			const uint32_t z = FZ * zo + (k >> 1), y = 2u * yo + (k & 1);
			if (z < p.nslices_in && y < g.sy) row[k].open(t, run_label, z, y, wo);
		}
		uint64_t* out = pool_label + cut_off[at];
		uint32_t rest = cut[at];
		while (rest) {
			const uint32_t j = __builtin_ctz(rest);
			rest &= rest - 1u;
			const bool two = 64u * wo + 2u * j + 1u < g.sx;      // the block's second column exists
			uint64_t v[2 * kRows];
#pragma unroll
			for (int k = 0; k < kRows; k++) {
				v[2 * k] = 0; v[2 * k + 1] = 0;
				if (row[k].on) row[k].pair(j, v[2 * k], v[2 * k + 1]);
			}
			uint64_t l;
			if constexpr (FZ == 1) {
				const uint64_t a = v[0], b = v[1], c = v[2], d = v[3];
				if (!two || !row[1].on) l = a;
				else l = (a == b || a == c) ? a : (b == c ? b : d);
			}
			else {
				l = 0;
				uint32_t best = 0;
#pragma unroll
				for (int k = 0; k < 2 * kRows; k++) {
					if (!row[k >> 1].on || ((k & 1) && !two)) continue;
					uint32_t times = 0;
#pragma unroll
					for (int m = 0; m < 2 * kRows; m++) times += row[m >> 1].on && (!(m & 1) || two) && v[m] == v[k];
					if (times > best || (times == best && v[k] < l)) { l = v[k]; best = times; }
				}
			}
			*out++ = l;
			mx = l > mx ? l : mx;
		}
	}
	block_max_into(mx, s_max, max_out);
}

// One thread per OUTPUT word: the pooled volume's planes V and H with the bits and the counts that
// k_label_planes_from_runs leaves (bits at or past sx, x = 0 of V and y = 0 of H stay 0; counts zeroed by the host: [osz]
// bits of V, [osz] bits of H, [osz] wrap pairs).  The word is cut at the cuts of the row itself and of the row above;
// inside a piece both rows have one label each.  The pixel before a word's first one, in x-fastest order, is the last
// pixel of the word before it in the [osz][plane_words] arrays.  t carries pool_cut, pool_off and pool_label.
// grid = (ceil(plane_words / 256), osz)
__global__ void __launch_bounds__(kBlock) k_pool_planes(
	RunLabels t, PoolGeom p, uint32_t* __restrict__ planeV, uint32_t* __restrict__ planeH, uint32_t* __restrict__ counts, uint32_t nslices
) {
	__shared__ uint32_t s_red[kWaves];
	const uint32_t zo = blockIdx.y;
	const uint64_t i = this_word();
	uint32_t nv = 0, nh = 0, nw = 0;
	if (i < p.plane_words) {
		const uint32_t y = static_cast<uint32_t>(i / p.row_words), w = static_cast<uint32_t>(i - static_cast<uint64_t>(y) * p.row_words);
		const uint32_t valid = p.valid_mask(w);
		const uint64_t at = zo * p.plane_words + i, up = at - p.row_words;      // (up: used with y >= 1 only)
		const uint32_t c = t.pool_cut[at], cu = y ? t.pool_cut[up] : 0u;
		const uint64_t* lab = t.pool_label + t.pool_off[at];
		const uint64_t* labu = t.pool_label + (y ? t.pool_off[up] : 0ull);
		uint64_t lc = at ? t.pool_label[t.pool_off[at - 1] + __popc(t.pool_cut[at - 1]) - 1u] : 0ull, lu = 0;
		if (w == 0 && at) nw = lc == lab[0];      // the row's first pixel against the pixel before it in x-fastest order
		uint32_t v = 0, h = 0;
		uint32_t rest = (c | cu) & valid;
		while (rest) {
			const uint32_t x = __builtin_ctz(rest);
			rest &= rest - 1u;
			if ((c >> x) & 1u) {
				const uint64_t l = *lab++;
				if ((w | x) && l != lc) v |= 1u << x;
				lc = l;
			}
			if (y) {
				if ((cu >> x) & 1u) lu = *labu++;
				if (lc != lu) h |= bits_from_to(x, rest ? __builtin_ctz(rest) : 32u);      // the piece ends at the next cut
			}
		}
		h &= valid;
		planeV[at] = v; planeH[at] = h;
		nv = __popc(v); nh = __popc(h);
	}
	add_plane_counts(nv, nh, nw, s_red, counts, nslices, zo);
}

}  // namespace dev
}  // namespace ckl
