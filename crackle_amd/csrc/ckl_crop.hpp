// ckl_crop: an x, y, z box of a stream as a stream of its own, without the voxels of either.  The road's first unit that
// serves many outputs from one TABLES run: the decode session is opened once over the z-range that the boxes of a call
// span, one label per run is gathered once, and every box then takes its own turn through the kernels below and the
// encoder.  As for downsample the word grid is the OUTPUT's (the box's PoolGeom), while everything read from the decode
// session is the input's (RunLabels::g); the box's origin (CropBox) is what ties the two together.
//
// A row of the box is a stretch of an input row, so its label changes exactly where the input row has a break inside
// the box.  Output word wo of box row (zo, yo) holds input columns c .. c + 31 with c = x0 + 32 wo of input row
// (zi0 + zo, y0 + yo): with wi = c >> 5 and sh = c & 31 its breaks are the funnel shift of input words wi and wi + 1 by
// sh.  The box's labels exist as the labelled cuts that ckl_downsample.hpp introduced, at the box's shape:
//   cut        [box depth][plane_words]  the input row's breaks under the word | bit 0 of every word
//   cut_off    [box depth][plane_words]  where the word's cuts stand in the label array (64-bit)
//   label      [cuts]                    the label from each cut up to the next one
// The kernels, in launch order:
//   k_erode_run_labels   (ckl_erode.hpp) once per CALL: one label per run of the session
//   k_crop_cuts          cut and cut_off, the scan and the cursor as k_pool_cuts has them
//   -- the cursor's final value, the number of cuts, crosses to the host, which sizes the label array --
//   k_crop_labels        a thread per word: the run of the word's first pixel by RunLabels' own formula (no carry from the
//                        word before it), one run further at every further cut; the largest label of the BOX is taken
//                        as k_pool_labels takes it (a box can lose the input's largest label)
//   k_pool_planes        (ckl_downsample.hpp, unchanged) with the box's PoolGeom, fz = 1: the first row, the first slice
//                        and the wrap-around pairs are the box's own
// The label stage then reads the triple through RunLabels::pooled (k_component_labels_from_runs), as for downsample.
#pragma once

#include "ckl_downsample.hpp"

namespace ckl {
namespace dev {

// a box inside the decode session's slices, and its own word grid
struct CropBox {
	uint32_t x0, y0, zi0;      // the box's first column, row and slice; the slice counts from the SESSION's first
	PoolGeom p;                // { 1, box depth, box width, box height, row_words, plane_words } of the box
};

// the breaks of input row (zi, y) in the 32 columns from column c on (c < g.sx): bit k is column c + k.  Input word
// (c >> 5) + 1 is read only where it exists, and nothing is shifted by 32.
__device__ __forceinline__ uint32_t crop_breaks(const RunGeom& g, uint32_t zi, uint32_t y, uint32_t c) {
	const uint32_t wi = c >> 5, sh = c & 31u;
	uint32_t b = g.breaks(zi, y, wi);
	if (sh) {
		const uint32_t next = wi + 1u < g.row_words ? g.breaks(zi, y, wi + 1u) : 0u;
		b = (b >> sh) | (next << (32u - sh));
	}
	return b;
}

// One thread per OUTPUT word: cut and cut_off (header comment).  *cursor zeroed by the host; afterwards it holds the
// number of cuts.  No thread leaves early: the scan is the workgroup's.  grid = (ceil(box.p.plane_words / 256), box depth)
__global__ void __launch_bounds__(kBlock) k_crop_cuts(
	RunGeom g, CropBox box, uint32_t* __restrict__ cut, uint64_t* __restrict__ cut_off, unsigned long long* __restrict__ cursor
) {
	__shared__ uint32_t s_scan[kWaves];
	__shared__ unsigned long long s_base;
	const PoolGeom& p = box.p;
	const uint32_t zo = blockIdx.y;
	const uint64_t i = this_word();
	const bool live = i < p.plane_words;
	const uint64_t at = zo * p.plane_words + i;
	uint32_t c = 0;
	if (live) {
		const uint32_t yo = static_cast<uint32_t>(i / p.row_words), wo = static_cast<uint32_t>(i - static_cast<uint64_t>(yo) * p.row_words);
		c = (crop_breaks(g, box.zi0 + zo, box.y0 + yo, box.x0 + 32u * wo) | 1u) & p.valid_mask(wo);
		cut[at] = c;
	}
	uint32_t v[1] = { static_cast<uint32_t>(__popc(c)) }, total[1];
	block_excl_add<1>(v, total, s_scan);
	if (threadIdx.x == 0) s_base = total[0] ? atomicAdd(cursor, static_cast<unsigned long long>(total[0])) : 0ull;
	__syncthreads();
	if (live) cut_off[at] = s_base + v[0];
}

// One thread per OUTPUT word: the label at each of its cuts -> label, and the largest of them (one atomicMax per
// workgroup; *max_out zeroed by the host).  Every run index is clamped to the slice's runs, as CombineRow::fetch clamps.
// grid = (ceil(box.p.plane_words / 256), box depth)
__global__ void __launch_bounds__(kBlock) k_crop_labels(
	RunLabels t, const uint64_t* __restrict__ run_label, CropBox box, const uint32_t* __restrict__ cut, const uint64_t* __restrict__ cut_off,
	uint64_t* __restrict__ label, unsigned long long* __restrict__ max_out
) {
	__shared__ unsigned long long s_max[kWaves];
	const PoolGeom& p = box.p;
	const uint32_t zo = blockIdx.y;
	const uint64_t i = this_word();
	unsigned long long mx = 0;
	if (i < p.plane_words) {
		const uint32_t yo = static_cast<uint32_t>(i / p.row_words), wo = static_cast<uint32_t>(i - static_cast<uint64_t>(yo) * p.row_words);
		const uint64_t at = zo * p.plane_words + i;
		const uint32_t zi = box.zi0 + zo, y = box.y0 + yo, c = box.x0 + 32u * wo;
		const uint32_t n = t.nruns[zi];
		const uint64_t* lab = run_label + t.rbase[zi];
		uint32_t run = t.run_at(zi, c, y);      // the run that holds the word's first pixel, wherever it began
		uint64_t* out = label + cut_off[at];
		uint32_t rest = cut[at];
		while (rest) {
			const uint32_t x = __builtin_ctz(rest);
			rest &= rest - 1u;
			if (x) run++;      // (bit 0 is the word's first pixel; every further cut is a break of the input row)
			const uint64_t l = n ? lab[run < n ? run : n - 1u] : 0ull;
			*out++ = l;
			mx = l > mx ? l : mx;
		}
	}
	block_max_into(mx, s_max, max_out);
}

}  // namespace dev
}  // namespace ckl
