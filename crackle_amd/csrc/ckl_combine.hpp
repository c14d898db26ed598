// ckl_combine: two streams of one shape merged by a rule on their labels, without the voxels of either.  The road's
// first unit with two inputs: two decode sessions stand side by side after their TABLES runs, and everything read from
// one of them goes through that session's own tables (CombineSide), because the two may differ in crack format, in runs
// and in components.
//
// The rules, with a the label of the first stream and b of the second at a voxel (b's value matters only as "is it 0"):
//   CKL_COMBINE_OVERLAY      b != 0 ? b : a
//   CKL_COMBINE_KEEP_WHERE   b != 0 ? a : 0
//   CKL_COMBINE_DROP_WHERE   b != 0 ? 0 : a
//
// The combined label of a row can change only where one of the two rows has a break, so the combined labels exist as
// the labelled cuts that ckl_downsample.hpp introduced, here at the volume's own shape:
//   cut        [nslices][plane_words]  breaks of the first stream | breaks of the second | bit 0 of every word
//   cut_off    [nslices][plane_words]  where the word's cuts stand in the label array (64-bit)
//   label      [cuts]                  the combined label from each cut up to the next one
// A cut is where the label MAY change: neighbouring entries can be equal.  The kernels, in launch order:
//   k_erode_run_labels   (ckl_erode.hpp) once per session: one label per run
//   k_combine_cuts       cut and cut_off, the scan and the cursor as k_pool_cuts has them
//   -- the cursor's final value, the number of cuts, crosses to the host, which sizes the label array --
//   k_combine_labels     a thread per word walks its cuts with one run cursor per stream; a stream's label is fetched
//                        once per run, at the run's break; the rule is evaluated at each cut; the largest stored label is
//                        taken as k_pool_labels takes it
//   k_pool_planes        (ckl_downsample.hpp, unchanged) with a PoolGeom of the volume's own shape, fz = 1
// The label stage then reads the triple through RunLabels::pooled (k_component_labels_from_runs), as for downsample.
#pragma once

#include "ckl_downsample.hpp"

namespace ckl {
namespace dev {

// what the kernels here read of one decode session: its crack planes, where its words' runs begin, and one label per run
// at the slices' own bases (k_erode_run_labels)
struct CombineSide {
	RunGeom g;
	const uint32_t* word_base;      // [nslices][plane_words]
	const uint64_t* rbase;          // per slice base into run_label
	const uint32_t* nruns;          // [nslices]
	const uint64_t* run_label;
};

// One thread per word: cut and cut_off (header comment).  The two RunGeoms agree in sx, sy, row_words and plane_words (the
// host has checked).  *cursor zeroed by the host; afterwards it holds the number of cuts.  No thread leaves early: the
// scan is the workgroup's.  grid = (ceil(plane_words / 256), nslices)
__global__ void __launch_bounds__(kBlock) k_combine_cuts(
	RunGeom ga, RunGeom gb, uint32_t* __restrict__ cut, uint64_t* __restrict__ cut_off, unsigned long long* __restrict__ cursor
) {
	__shared__ uint32_t s_scan[kWaves];
	__shared__ unsigned long long s_base;
	const uint32_t zi = blockIdx.y;
	const uint64_t i = this_word();
	const bool live = i < ga.plane_words;
	const uint64_t at = zi * ga.plane_words + i;
	uint32_t c = 0;
	if (live) {
		const PlaneWord pw(ga, zi, i);
		c = (ga.breaks(zi, pw.y, pw.w) | gb.breaks(zi, pw.y, pw.w) | 1u) & pw.valid;
		cut[at] = c;
	}
	uint32_t v[1] = { static_cast<uint32_t>(__popc(c)) }, total[1];
	block_excl_add<1>(v, total, s_scan);
	if (threadIdx.x == 0) s_base = total[0] ? atomicAdd(cursor, static_cast<unsigned long long>(total[0])) : 0ull;
	__syncthreads();
	if (live) cut_off[at] = s_base + v[0];
}

// one stream's row under a word: its breaks in the word, its run cursor and the label of the run the cursor stands on.
// Every run index is clamped to the slice's runs, as PoolRow::fetch clamps.
struct CombineRow {
	uint32_t b, n, run;
	const uint64_t* lab;
	uint64_t carry = 0;
	__device__ __forceinline__ uint64_t fetch(uint32_t r) const { return n ? lab[r < n ? r : n - 1u] : 0ull; }
	__device__ __forceinline__ CombineRow(const CombineSide& t, uint32_t zi, const PlaneWord& pw)
		: b(t.g.breaks(zi, pw.y, pw.w)), n(t.nruns[zi]), run(t.word_base[pw.at] - 1u), lab(t.run_label + t.rbase[zi]) {      // run: the one that reaches into the word from the left
		if (!(b & 1u)) carry = fetch(run);      // (w = 0 has bit 0 set)
	}
	// the label at pixel x of the word; called with ascending x, at every x where b has a bit (and wherever else: without
	// a bit it is the label carried over)
	__device__ __forceinline__ uint64_t at(uint32_t x) {
		if ((b >> x) & 1u) carry = fetch(++run);
		return carry;
	}
};

template <int RULE>
__device__ __forceinline__ uint64_t combine_rule(uint64_t a, uint64_t b) {
	if constexpr (RULE == CKL_COMBINE_OVERLAY) return b ? b : a;
	else if constexpr (RULE == CKL_COMBINE_KEEP_WHERE) return b ? a : 0ull;
	else return b ? 0ull : a;
}

// One thread per word: the combined label at each of its cuts -> label, and the largest of them (one atomicMax per
// workgroup; *max_out zeroed by the host).  grid = (ceil(plane_words / 256), nslices)
template <int RULE>
__global__ void __launch_bounds__(kBlock) k_combine_labels(
	CombineSide ta, CombineSide tb, const uint32_t* __restrict__ cut, const uint64_t* __restrict__ cut_off,
	uint64_t* __restrict__ label, unsigned long long* __restrict__ max_out
) {
	__shared__ unsigned long long s_max[kWaves];
	const uint32_t zi = blockIdx.y;
	const uint64_t i = this_word();
	unsigned long long mx = 0;
	if (i < ta.g.plane_words) {
		const PlaneWord pw(ta.g, zi, i);
		CombineRow ra(ta, zi, pw), rb(tb, zi, pw);
		uint64_t* out = label + cut_off[pw.at];
		uint32_t rest = cut[pw.at];
		while (rest) {
			const uint32_t x = __builtin_ctz(rest);
			rest &= rest - 1u;
			const uint64_t a = ra.at(x), b = rb.at(x);      // (both cursors move at every cut: no short circuit)
			const uint64_t l = combine_rule<RULE>(a, b);
			*out++ = l;
			mx = l > mx ? l : mx;
		}
	}
	block_max_into(mx, s_max, max_out);
}

}  // namespace dev
}  // namespace ckl
