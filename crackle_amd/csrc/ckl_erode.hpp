// ckl_erode: the labels of a stream eroded by one voxel, without its voxels.  A voxel keeps its label L != 0 when
// every neighbour of the structuring element (6, 18 or 26 neighbours) carries L; every other voxel becomes 0.  The
// keep bit K of every pixel is a function of (runs, label of every run), as everything in ckl_recompress.hpp is, and
// the eroded volume's "differs from the neighbour" planes are K ^ K(x - 1) and K ^ K(y - 1): all three elements hold
// the four in-plane face neighbours, so two kept neighbours share a label and a kept pixel differs from an unkept one
// (which is 0).  The kernels, in launch order:
//   k_erode_run_labels   one label per run (run -> component -> label gathered once, not once per neighbour row)
//   k_erode_terms        per 32-pixel word the bit planes P, C, D that K is made of
//   k_erode_keep         K from P, C, D of the word and of its two neighbours in the row; the largest surviving label
//   k_erode_planes       the encoder's V and H planes from K, their per-slice counts and the wrap-around pairs
// The label stage then reads K through RunLabels::keep (k_component_labels_from_runs).
//
// With Q1(x): label(x) != 0 and the four face rows (dy, dz) = (+-1, 0), (0, +-1) carry the same label in column x,
//      Q2(x): the four diagonal rows (+-1, +-1) carry the same label in column x,
//      D(x):  label(x) == label(x - 1) in the row itself,
//    6:  K(x) = Q1(x)                                               & D(x) & D(x + 1)
//   18:  K(x) = Q1(x - 1) & Q1(x) & Q1(x + 1) & Q2(x)               & D(x) & D(x + 1)
//   26:  K(x) = Q1(x - 1) & Q1(x) & Q1(x + 1) & Q2(x - 1 .. x + 1)  & D(x) & D(x + 1)
// so P (the term taken at x - 1, x and x + 1) is Q1 at 18 and Q1 & Q2 at 26, C (taken at x alone) is Q1 at 6 and
// Q1 & Q2 at 18 and 26.  A row or column outside the volume: its term is 1 (CKL_ERODE_KEEP_BORDER), or the pixel goes.
#pragma once

#include "ckl_recompress.hpp"

namespace ckl {
namespace dev {

struct ErodeArgs {
	uint32_t connectivity;      // 6, 18, 26
	uint32_t keep_border;       // neighbours outside the volume are ignored
	uint32_t nslices;
};

// run_label[rbase[zi] + run] = label of run `run` of slice zi.  grid = (any, nslices), grid-stride over the runs
__global__ void __launch_bounds__(kBlock) k_erode_run_labels(RunLabels t, uint64_t* __restrict__ run_label) {
	const uint32_t zi = blockIdx.y;
	const uint32_t n = t.nruns[zi];
	const uint32_t nce = t.ncomp[zi];
	const uint32_t* rcc = t.run_cc + t.rbase[zi];
	const uint64_t* lmap = t.label_map + t.comp_off[zi];
	uint64_t* out = run_label + t.rbase[zi];
	for (uint32_t run = blockIdx.x * kBlock + threadIdx.x; run < n; run += gridDim.x * kBlock) {
		const uint32_t cc = rcc[run];
		out[run] = cc < nce ? lmap[cc] : 0ull;
	}
}

// the labels of one slice's runs, every index clamped to the slice's runs
struct SliceRunLabels {
	const uint64_t* lab;
	uint32_t n;
	__device__ __forceinline__ SliceRunLabels(const RunLabels& t, const uint64_t* run_label, uint32_t zi) : lab(run_label + t.rbase[zi]), n(t.nruns[zi]) {}
	__device__ __forceinline__ uint64_t operator()(uint32_t run) const { return n ? lab[run < n ? run : n - 1u] : 0ull; }
};

// One walk over the runs of word `p` of slice zi (b: its breaks), one label fetch per run.  Returns the bits of the
// pixels whose label is not 0; same_as_before: bit x set where pixel x carries the label of the pixel before it in the
// row (x = 0 of the row: set).  Bits at or past sx are 0 in both.  (k_dilate_nonzero has no use for the second word.)
__device__ __forceinline__ uint32_t nonzero_bits(const RunLabels& t, const uint64_t* run_label, uint32_t zi, const PlaneWord& p, uint32_t b, uint32_t& same_as_before) {
	const SliceRunLabels lab(t, run_label, zi);
	uint32_t rc = t.word_base[p.at] - 1u;      // the run that reaches into the word from the left
	uint64_t lc = p.w ? lab(rc) : 0ull;
	uint32_t nz = 0, d = p.valid;
	uint32_t rest = (b | 1u) & p.valid;
	while (rest) {
		const uint32_t x = __builtin_ctz(rest);
		rest &= rest - 1u;
		if ((b >> x) & 1u) {
			const uint64_t l = lab(++rc);
			if ((p.w | x) && l != lc) d &= ~(1u << x);
			lc = l;
		}
		if (lc) nz |= bits_from_to(x, rest ? __builtin_ctz(rest) : 32u);
	}
	same_as_before = d;
	return nz & p.valid;
}

// bit x set: pixel x of word w carries the same label in row (yc, zc) and in row (yn, zn).  The word is cut at the
// breaks of both rows; inside a piece both rows have one label each.
__device__ __forceinline__ uint32_t same_label_bits(
	const RunLabels& t, const uint64_t* run_label, uint32_t zc, uint32_t yc, uint32_t bc, uint32_t zn, uint32_t yn, uint32_t w, uint32_t valid
) {
	const RunGeom& g = t.g;
	const SliceRunLabels labc(t, run_label, zc), labn(t, run_label, zn);
	const uint32_t bn = g.breaks(zn, yn, w);
	uint32_t rc = t.word_base[zc * g.plane_words + static_cast<uint64_t>(yc) * g.row_words + w] - 1u;      // the run that reaches into the word from the left
	uint32_t rn = t.word_base[zn * g.plane_words + static_cast<uint64_t>(yn) * g.row_words + w] - 1u;
	uint64_t lc = 0, ln = 0;
	if (!(bc & 1u)) lc = labc(rc);      // (w = 0 has bit 0 set in both)
	if (!(bn & 1u)) ln = labn(rn);
	uint32_t eq = 0;
	uint32_t rest = (bc | bn | 1u) & valid;
	while (rest) {
		const uint32_t x = __builtin_ctz(rest);
		rest &= rest - 1u;
		if ((bc >> x) & 1u) lc = labc(++rc);
		if ((bn >> x) & 1u) ln = labn(++rn);
		if (lc == ln) eq |= bits_from_to(x, rest ? __builtin_ctz(rest) : 32u);
	}
	return eq & valid;
}

// One thread per 32-pixel word (zi, y, w): the planes P, C, D of the header comment, [nslices][plane_words] each.
// D's bit of x = 0 is 1 (there is no pixel before it; k_erode_keep applies the border rule in x).  Bits at or past sx
// are 0.  grid = (ceil(plane_words / 256), nslices)
__global__ void __launch_bounds__(kBlock) k_erode_terms(
	RunLabels t, const uint64_t* __restrict__ run_label, ErodeArgs a, uint32_t* __restrict__ planeP, uint32_t* __restrict__ planeC, uint32_t* __restrict__ planeD
) {
	const RunGeom& g = t.g;
	const uint32_t zi = blockIdx.y;
	const uint64_t i = this_word();
	if (i >= g.plane_words) return;
	const PlaneWord pw(g, zi, i);
	const uint32_t y = pw.y, w = pw.w, valid = pw.valid;
	const uint64_t at = pw.at;
	const uint32_t b = g.breaks(zi, y, w);
	// the row itself: where the label is not 0, and where it equals the pixel before
	uint32_t d;
	const uint32_t nz = nonzero_bits(t, run_label, zi, pw, b, d);
	// the neighbour rows: k = 0 .. 3 the face rows, 4 .. 7 the diagonal ones
	uint32_t q1 = nz, q2 = valid;
	const uint32_t nrows = a.connectivity == 6u ? 4u : 8u;
#pragma unroll 1
	for (uint32_t k = 0; k < nrows && q1; k++) {
		int dy, dz;
		if (k < 4u) { dy = k == 0u ? -1 : (k == 1u ? 1 : 0); dz = k == 2u ? -1 : (k == 3u ? 1 : 0); }
		else { dy = (k & 1u) ? 1 : -1; dz = (k & 2u) ? 1 : -1; }
		const int64_t yn = static_cast<int64_t>(y) + dy, zn = static_cast<int64_t>(zi) + dz;
		uint32_t eq;
		if (yn < 0 || yn >= static_cast<int64_t>(g.sy) || zn < 0 || zn >= static_cast<int64_t>(a.nslices)) eq = a.keep_border ? valid : 0u;
		else eq = same_label_bits(t, run_label, zi, y, b, static_cast<uint32_t>(zn), static_cast<uint32_t>(yn), w, valid);
		if (k < 4u) q1 &= eq;
		else q2 &= eq;
	}
	const uint32_t q12 = q1 & q2;
	planeP[at] = a.connectivity == 26u ? q12 : q1;
	planeC[at] = a.connectivity == 6u ? q1 : q12;
	planeD[at] = d;
}

// One thread per word: K, and the largest label of a kept pixel (one atomicMax per workgroup; *max_out zeroed by the
// host).  P(x - 1), P(x + 1) and D(x + 1) come from the neighbouring words by funnel shifts; outside the row they are 1,
// and without keep_border the row's first and last pixel go instead.  grid = (ceil(plane_words / 256), nslices)
__global__ void __launch_bounds__(kBlock) k_erode_keep(
	RunLabels t, const uint64_t* __restrict__ run_label, ErodeArgs a, const uint32_t* __restrict__ planeP, const uint32_t* __restrict__ planeC,
	const uint32_t* __restrict__ planeD, uint32_t* __restrict__ keep, unsigned long long* __restrict__ max_out
) {
	__shared__ unsigned long long s_max[kWaves];
	const RunGeom& g = t.g;
	const uint32_t zi = blockIdx.y;
	const uint64_t i = this_word();
	unsigned long long mx = 0;
	if (i < g.plane_words) {
		const auto [y, w, valid, at] = PlaneWord(g, zi, i);
		const bool first = w == 0u, last = w + 1u == g.row_words;
		const uint32_t d = planeD[at] | ~valid;
		const uint32_t dn = last ? 0xFFFFFFFFu : planeD[at + 1];
		uint32_t k = planeC[at] & d & ((d >> 1) | (dn << 31));
		if (a.connectivity != 6u) {
			const uint32_t p = planeP[at] | ~valid;
			const uint32_t pl = first ? 0xFFFFFFFFu : planeP[at - 1];
			const uint32_t pn = last ? 0xFFFFFFFFu : planeP[at + 1];
			k &= ((p << 1) | (pl >> 31)) & ((p >> 1) | (pn << 31));
		}
		k &= valid;
		if (!a.keep_border) {
			if (first) k &= ~1u;
			if (last) k &= ~(1u << ((g.sx - 1u) & 31u));
		}
		keep[at] = k;
		if (k) {
			// one label per run that has a kept pixel
			const SliceRunLabels lab(t, run_label, zi);
			const uint32_t b = g.breaks(zi, y, w);
			const uint32_t rc = t.word_base[at] - 1u;
			uint32_t rest = k;
			while (rest) {
				const uint32_t x = __builtin_ctz(rest);
				const unsigned long long l = lab(rc + __popc(b & mask_le(x)));
				mx = l > mx ? l : mx;
				const uint32_t next = b & ~mask_le(x);      // the run ends at the next break
				rest &= ~bits_from_to(0u, next ? __builtin_ctz(next) : 32u);
			}
		}
	}
	block_max_into(mx, s_max, max_out);
}

// One thread per word: the eroded volume's planes V = K ^ K(x - 1) and H = K ^ K(y - 1), with the bits and the counts
// that k_label_planes_from_runs leaves (bits at or past sx, x = 0 of V and y = 0 of H stay 0; counts zeroed by the
// host: [nslices] bits of V, [nslices] bits of H, [nslices] wrap pairs).  The first pixel of a row equals the pixel
// before it in x-fastest order when both are unkept, or both are kept and carry one label (they are no neighbours in
// the volume, so two kept ones may differ).  grid = (ceil(plane_words / 256), nslices)
__global__ void __launch_bounds__(kBlock) k_erode_planes(
	RunLabels t, const uint64_t* __restrict__ run_label, const uint32_t* __restrict__ keep, uint32_t* __restrict__ planeV, uint32_t* __restrict__ planeH,
	uint32_t* __restrict__ counts, uint32_t nslices
) {
	__shared__ uint32_t s_red[kWaves];
	const RunGeom& g = t.g;
	const uint32_t zi = blockIdx.y;
	const uint64_t i = this_word();
	uint32_t nv = 0, nh = 0, nw = 0;
	if (i < g.plane_words) {
		const auto [y, w, valid, at] = PlaneWord(g, zi, i);
		const uint32_t k = keep[at];
		const uint32_t kl = w ? keep[at - 1] : 0u;
		uint32_t v = (k ^ ((k << 1) | (kl >> 31))) & valid;
		if (w == 0) v &= ~1u;
		const uint32_t h = y ? ((k ^ keep[at - g.row_words]) & valid) : 0u;
		if (w == 0 && (y | zi)) {
			const uint32_t zp = y ? zi : zi - 1u, yp = y ? y - 1u : g.sy - 1u, xp = g.sx - 1u;
			const uint32_t kp = (keep[zp * g.plane_words + static_cast<uint64_t>(yp) * g.row_words + (xp >> 5)] >> (xp & 31u)) & 1u;
			const uint32_t kc = k & 1u;
			if (!kp && !kc) nw = 1u;
			else if (kp && kc) nw = SliceRunLabels(t, run_label, zp)(t.run_at(zp, xp, yp)) == SliceRunLabels(t, run_label, zi)(t.run_at(zi, 0u, y));
		}
		planeV[at] = v; planeH[at] = h;
		nv = __popc(v); nh = __popc(h);
	}
	add_plane_counts(nv, nh, nw, s_red, counts, nslices, zi);
}

}  // namespace dev
}  // namespace ckl
