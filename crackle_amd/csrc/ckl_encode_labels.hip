// The encoder's flat label stage (declared in ckl_encode_labels.hpp; its state is the session's LabelStage, ckl_encoder.hpp):
//   cc3d::connected_components2d_4 + relabel        src/cc3d.hpp:114-144, 257-369        ckl_strips.hpp (strips of the label planes), ckl_runs.hpp (runs)
//   labels::encode_flat                             src/labels.hpp:30-155      k_run_resolve / k_slice_resolve_enc (crc), k_mapping_comps / k_gather_slots + hash / sort / unique, k_flat_section
// Everything here runs on the session's label stream (stream2).  The encoder's schedule (ckl_encode.hip) decides when it
// starts; crackle.operations.recompress without the voxels (ckl_recompress.hip) has the stage launch
// k_component_labels_from_runs (ckl_recompress.hpp) in place of the kernels that read a volume.
#include "ckl_encode_labels.hpp"
#include "ckl_runs.hpp"
#include "ckl_strips.hpp"
#include "ckl_recompress.hpp"

#include <algorithm>

using namespace ckl;
using namespace ckl::dev;

namespace {

// ------------------------------------------------------------------------------
// flat labels (labels.hpp:56-88): component -> label, read at the first pixel of every
// component.  grid = (ceil(max components of a slice / 256), nslices)
// ------------------------------------------------------------------------------
// component -> label from the component's first pixel (k_run_assign leaves it in comp_pix): one thread per
// component instead of one per run (C2: 1.6 M instead of 26 M)
template <typename LABEL>
__global__ void __launch_bounds__(kBlock) k_mapping_comps(
	const LABEL* __restrict__ labels, RunArrays r, uint64_t sxy,
	const uint64_t* __restrict__ comp_off, uint64_t* __restrict__ mapping
) {
	const uint32_t zi = blockIdx.y;
	const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
	if (c >= r.ncomp[zi]) return;
	mapping[comp_off[zi] + c] = static_cast<uint64_t>(labels[zi * sxy + r.comp_pix[r.rbase[zi] + c]]);
}

// the encoder's strips (flat_enqueue): planes only, no record lists; seven workgroups per CU like k_strip_ccl
// Tables of kEncStripCap runs, not kStripCap: the label stream runs beside two walks per CU and has kFlatResolveLds of
// the CU's LDS (label_start, ckl_encode.hip).  Two of these workgroups fit into that, of the decoder's size only one:
// at C2 (two walks of 58 KiB) the kernel took 0.79 ms with 2560 runs and the encode was slower than on the run pipeline;
// with 2048, although the strips get 28 rows instead of 32, the encode's device time went from 2.72 to 2.56 ms.
constexpr uint32_t kEncStripCap = 2048;
static_assert(2 * strip_ccl_words(kEncStripCap) * sizeof(uint32_t) <= kFlatResolveLds, "two strip workgroups beside two walks");
__global__ void __launch_bounds__(kBlock, 7) k_strip_ccl_enc(RunGeom g, StripArrays sa, const uint32_t* __restrict__ G, uint32_t n_pixels) {
	__shared__ __attribute__((aligned(16))) uint32_t s_lds[strip_ccl_words(kEncStripCap)];
	strip_ccl_body<false, false, true, kEncStripCap>(g, sa, RecordLists{}, G, n_pixels, nullptr, blockIdx.y, blockIdx.x, s_lds);
}

// one thread per component: the slots of k_slice_resolve_enc -> the dense table (comp_off: the host's prefix of the
// counts).  grid = (ceil(max components / kBlock), slices)
__global__ void __launch_bounds__(kBlock) k_gather_slots(
	const uint64_t* __restrict__ slots, uint32_t slot_cap, const uint32_t* __restrict__ ncomp, const uint64_t* __restrict__ comp_off, uint64_t* __restrict__ mapping
) {
	const uint32_t zi = blockIdx.y;
	const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
	if (c < ncomp[zi]) mapping[comp_off[zi] + c] = slots[static_cast<uint64_t>(zi) * slot_cap + c];
}

// Global component id of every voxel (cc3d.hpp:371-400 numbers components continuously
// across slices) for the pin encoder: one thread per pixel, its run found by a popcount in
// the row's break word, ids read from the run tables.  grid = (ceil(sxy / 256), nslices)
__global__ void __launch_bounds__(kBlock) k_paint_components(
	const uint32_t* __restrict__ planeV, uint32_t row_words, uint64_t plane_words, uint32_t sx, uint64_t sxy,
	const uint32_t* __restrict__ word_base, const uint64_t* __restrict__ rbase, const uint32_t* __restrict__ run_cc,
	const uint64_t* __restrict__ comp_off, uint32_t id_base, uint32_t* __restrict__ out
) {
	const uint32_t zi = blockIdx.y;
	const uint32_t px = blockIdx.x * kBlock + threadIdx.x;
	if (px >= sxy) return;
	const uint32_t y = px / sx, x = px - y * sx;
	const uint32_t w = x >> 5, bit = x & 31u;
	const uint64_t wi = zi * plane_words + static_cast<uint64_t>(y) * row_words + w;
	uint32_t b = planeV[wi];
	if (w == 0) b |= 1u;
	// word_base counts the runs that start before this word; bit i set = a run starts at pixel i
	const uint32_t run = word_base[wi] - 1u + __popc(b & (0xFFFFFFFFu >> (31u - bit)));
	out[zi * sxy + px] = run_cc[rbase[zi] + run] + static_cast<uint32_t>(comp_off[zi]) + id_base;
}

// The same with four pixels (16 bytes of ids) per thread: rows whose length is a multiple of four, where the four
// share a break word.  (4.1 ms -> for 2048 x 2048 x 256: one 4-byte store per lane moved 1 TB/s.)
__global__ void __launch_bounds__(kBlock) k_paint_components4(
	const uint32_t* __restrict__ planeV, uint32_t row_words, uint64_t plane_words, uint32_t sx, uint64_t sxy,
	const uint32_t* __restrict__ word_base, const uint64_t* __restrict__ rbase, const uint32_t* __restrict__ run_cc,
	const uint64_t* __restrict__ comp_off, uint32_t id_base, uint32_t* __restrict__ out
) {
	const uint32_t zi = blockIdx.y;
	const uint32_t px = (blockIdx.x * kBlock + threadIdx.x) * 4u;
	if (px >= sxy) return;
	const uint32_t y = px / sx, x = px - y * sx;
	const uint32_t w = x >> 5, bit = x & 31u;
	const uint64_t wi = zi * plane_words + static_cast<uint64_t>(y) * row_words + w;
	uint32_t b = planeV[wi];
	if (w == 0) b |= 1u;
	const uint32_t* cc = run_cc + rbase[zi];
	const uint32_t add = static_cast<uint32_t>(comp_off[zi]) + id_base;
	uint32_t run = word_base[wi] - 1u + __popc(b & (0xFFFFFFFFu >> (31u - bit)));
	uint4 o;
	o.x = cc[run] + add;
	run += (b >> (bit + 1u)) & 1u; o.y = cc[run] + add;
	run += (b >> (bit + 2u)) & 1u; o.z = cc[run] + add;
	run += (b >> (bit + 3u)) & 1u; o.w = cc[run] + add;
	*reinterpret_cast<uint4*>(out + zi * sxy + px) = o;
}

inline void launch_paint_components(hipStream_t s, const uint32_t* planeV, uint32_t row_words, uint64_t plane_words, int64_t sx, int64_t sy, int64_t sz,
	const uint32_t* word_base, const uint64_t* rbase, const uint32_t* run_cc, const uint64_t* comp_off, uint32_t id_base, uint32_t* out) {
	const uint64_t sxy = static_cast<uint64_t>(sx) * sy;
	const bool four = sx % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
	const uint64_t threads = four ? sxy / 4 : sxy;
	const dim3 grid(static_cast<uint32_t>((threads + kBlock - 1) / kBlock), static_cast<uint32_t>(sz));
	if (four) hipLaunchKernelGGL(k_paint_components4, grid, dim3(kBlock), 0, s, planeV, row_words, plane_words, static_cast<uint32_t>(sx), sxy, word_base, rbase, run_cc, comp_off, id_base, out);
	else hipLaunchKernelGGL(k_paint_components, grid, dim3(kBlock), 0, s, planeV, row_words, plane_words, static_cast<uint32_t>(sx), sxy, word_base, rbase, run_cc, comp_off, id_base, out);
}

// ------------------------------------------------------------------------------
// label table (labels.hpp:92-152): sorted unique labels and the key of every component.
// The component -> label list is sorted on device (bitonic network over a power-of-two
// padded copy), uniqued on the host in one linear pass, and the keys are found by binary
// search on device and packed at their byte width.
// ------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_bitonic_step(uint64_t* __restrict__ a, uint32_t j, uint32_t k, uint32_t n) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n) return;
	const uint32_t l = i ^ j;
	if (l > i) {
		const uint64_t x = a[i], y = a[l];
		const bool up = (i & k) == 0;
		if ((x > y) == up) { a[i] = y; a[l] = x; }
	}
}
// all steps with j < 2048 of one k-stage inside LDS (2048 elements per workgroup)
// every stage k = 2 .. 2048 of the network inside blocks of 2048 keys: one launch instead of eleven
// two steps of the network (distances j and j / 2) in one launch: a thread takes the four elements that the two
// steps exchange among themselves (the launches of the sort are what it costs: ~6 us each on the label stream)
__global__ void __launch_bounds__(kBlock) k_bitonic_step2(uint64_t* __restrict__ a, uint32_t j, uint32_t k, uint32_t n) {
	const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
	if (t >= n / 4u) return;
	const uint32_t h = j >> 1;
	const uint32_t lb = static_cast<uint32_t>(__ffs(h)) - 1u;
	const uint32_t i = (t & (h - 1u)) | ((t >> lb) << (lb + 2u));      // bits h and j clear
	uint64_t v0 = a[i], v1 = a[i | h], v2 = a[i | j], v3 = a[i | j | h];
	const bool up = (i & k) == 0;
	auto cx = [&](uint64_t& x, uint64_t& y) { if ((x > y) == up) { const uint64_t z = x; x = y; y = z; } };
	cx(v0, v2); cx(v1, v3);
	cx(v0, v1); cx(v2, v3);
	a[i] = v0; a[i | h] = v1; a[i | j] = v2; a[i | j | h] = v3;
}

__global__ void __launch_bounds__(kBlock) k_bitonic_first(uint64_t* __restrict__ a, uint32_t n) {
	__shared__ uint64_t s[2048];
	const uint32_t base = blockIdx.x * 2048u;
	for (uint32_t t = threadIdx.x; t < 2048u; t += kBlock) s[t] = base + t < n ? a[base + t] : ~0ull;
	__syncthreads();
	for (uint32_t k = 2; k <= 2048u; k <<= 1) {
		for (uint32_t j = k >> 1; j > 0; j >>= 1) {
			for (uint32_t t = threadIdx.x; t < 2048u; t += kBlock) {
				const uint32_t l = t ^ j;
				if (l > t) {
					const uint64_t x = s[t], y = s[l];
					const bool up = ((base + t) & k) == 0;
					if ((x > y) == up) { s[t] = y; s[l] = x; }
				}
			}
			__syncthreads();
		}
	}
	for (uint32_t t = threadIdx.x; t < 2048u; t += kBlock) if (base + t < n) a[base + t] = s[t];
}
__global__ void __launch_bounds__(kBlock) k_bitonic_local(uint64_t* __restrict__ a, uint32_t j_start, uint32_t k, uint32_t n) {
	__shared__ uint64_t s[2048];
	const uint32_t base = blockIdx.x * 2048u;
	for (uint32_t t = threadIdx.x; t < 2048u; t += kBlock) s[t] = base + t < n ? a[base + t] : ~0ull;
	__syncthreads();
	for (uint32_t j = j_start; j > 0; j >>= 1) {
		for (uint32_t t = threadIdx.x; t < 2048u; t += kBlock) {
			const uint32_t l = t ^ j;
			if (l > t) {
				const uint64_t x = s[t], y = s[l];
				const bool up = ((base + t) & k) == 0;
				if ((x > y) == up) { s[t] = y; s[l] = x; }
			}
		}
		__syncthreads();
	}
	for (uint32_t t = threadIdx.x; t < 2048u; t += kBlock) if (base + t < n) a[base + t] = s[t];
}
__global__ void __launch_bounds__(kBlock) k_pad_copy_u64(const uint64_t* __restrict__ src, uint64_t n, uint64_t* __restrict__ dst, uint64_t n_pad) {
	const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
	if (i < n_pad) dst[i] = i < n ? src[i] : ~0ull;
}
// sorted[N] -> uniq[U] (first of every run of equal values), U: heads counted per 2048-item
// block, block counts scanned by one workgroup, heads scattered.
constexpr uint32_t kUniqPer = 8, kUniqItems = kBlock * kUniqPer;
__device__ __forceinline__ uint32_t unique_heads(const uint64_t* __restrict__ sorted, uint32_t n, uint32_t i0, uint64_t (&v)[kUniqPer]) {
	uint32_t flag = 0;
#pragma unroll
	for (uint32_t q = 0; q < kUniqPer; q++) {
		const uint32_t i = i0 + q;
		v[q] = i < n ? sorted[i] : 0;
		const uint64_t prev = q ? v[q - 1] : ((i > 0 && i < n) ? sorted[i - 1] : 0);
		flag |= ((i < n && (i == 0 || v[q] != prev)) ? 1u : 0u) << q;
	}
	return flag;
}
// grid = ceil(n / 2048)
__global__ void __launch_bounds__(kBlock) k_unique_count(const uint64_t* __restrict__ sorted, uint32_t n, uint32_t* __restrict__ blk_count) {
	__shared__ uint32_t s_red[kWaves];
	uint64_t v[kUniqPer];
	const uint32_t flag = unique_heads(sorted, n, blockIdx.x * kUniqItems + threadIdx.x * kUniqPer, v);
	const uint32_t tot = block_sum(static_cast<uint32_t>(__popc(flag)), s_red);
	if (threadIdx.x == 0) blk_count[blockIdx.x] = tot;
}
// one workgroup: exclusive prefix of the block counts (in place) and the total
__global__ void __launch_bounds__(kBlock) k_unique_scan(uint32_t* __restrict__ blk_count, uint32_t nblk, uint32_t* __restrict__ n_uniq) {
	__shared__ uint32_t s_scan[kWaves];
	uint32_t carry = 0;
	for (uint32_t b0 = 0; b0 < nblk; b0 += kBlock) {
		const uint32_t b = b0 + threadIdx.x;
		uint32_t c[1] = { b < nblk ? blk_count[b] : 0u }, tot[1];
		block_excl_add<1>(c, tot, s_scan);
		if (b < nblk) blk_count[b] = carry + c[0];
		carry += tot[0];
	}
	if (threadIdx.x == 0) *n_uniq = carry;
}
// grid = ceil(n / 2048)
__global__ void __launch_bounds__(kBlock) k_unique_scatter(const uint64_t* __restrict__ sorted, uint32_t n, const uint32_t* __restrict__ blk_base, uint64_t* __restrict__ uniq) {
	__shared__ uint32_t s_scan[kWaves];
	uint64_t v[kUniqPer];
	const uint32_t flag = unique_heads(sorted, n, blockIdx.x * kUniqItems + threadIdx.x * kUniqPer, v);
	uint32_t c[1] = { static_cast<uint32_t>(__popc(flag)) }, tot[1];
	block_excl_add<1>(c, tot, s_scan);
	uint32_t o = blk_base[blockIdx.x] + c[0];
#pragma unroll
	for (uint32_t q = 0; q < kUniqPer; q++) if ((flag >> q) & 1u) uniq[o++] = v[q];
}

// The component labels are first reduced to their distinct values (a volume has far fewer labels
// than components: C2 has 1.6 M components and 65 k labels), so that only those are sorted: an
// open-addressing table keyed by label, then the occupied slots compacted like the unique heads
// above.  The all-ones label doubles as the empty marker and is noted in a flag of its own.
constexpr uint64_t kLabelHashEmpty = ~0ull;
__device__ __forceinline__ uint32_t label_hash(uint64_t v) {
	v ^= v >> 33; v *= 0xff51afd7ed558ccdull; v ^= v >> 33;
	return static_cast<uint32_t>(v);
}
// grid = ceil(n / 256); table: mask + 1 slots, preset to kLabelHashEmpty
__global__ void __launch_bounds__(kBlock) k_label_hash_insert(const uint64_t* __restrict__ mapping, uint32_t n, unsigned long long* __restrict__ table, uint32_t mask, uint32_t* __restrict__ has_max) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n) return;
	const unsigned long long v = mapping[i];
	if (v == kLabelHashEmpty) { *has_max = 1u; return; }
	uint32_t h = label_hash(v) & mask;
	for (uint32_t probe = 0; probe <= mask; probe++) {
		const unsigned long long seen = table[h];      // most components find their label already there
		if (seen == v) return;
		if (seen == kLabelHashEmpty) {
			const unsigned long long old = atomicCAS(table + h, kLabelHashEmpty, v);
			if (old == kLabelHashEmpty || old == v) return;
		}
		h = (h + 1u) & mask;
	}
}
__device__ __forceinline__ uint32_t hash_occupied(const unsigned long long* __restrict__ table, uint32_t slots, uint32_t i0, uint64_t (&v)[kUniqPer]) {
	uint32_t flag = 0;
#pragma unroll
	for (uint32_t q = 0; q < kUniqPer; q++) {
		v[q] = i0 + q < slots ? table[i0 + q] : kLabelHashEmpty;
		flag |= (v[q] != kLabelHashEmpty ? 1u : 0u) << q;
	}
	return flag;
}
// grid = ceil(slots / 2048)
__global__ void __launch_bounds__(kBlock) k_label_hash_count(const unsigned long long* __restrict__ table, uint32_t slots, uint32_t* __restrict__ blk_count) {
	__shared__ uint32_t s_red[kWaves];
	uint64_t v[kUniqPer];
	const uint32_t flag = hash_occupied(table, slots, blockIdx.x * kUniqItems + threadIdx.x * kUniqPer, v);
	const uint32_t tot = block_sum(static_cast<uint32_t>(__popc(flag)), s_red);
	if (threadIdx.x == 0) blk_count[blockIdx.x] = tot;
}
// grid = ceil(slots / 2048); the all-ones label, if seen, goes behind the others
__global__ void __launch_bounds__(kBlock) k_label_hash_scatter(
	const unsigned long long* __restrict__ table, uint32_t slots, const uint32_t* __restrict__ blk_base, const uint32_t* __restrict__ n_found,
	const uint32_t* __restrict__ has_max, uint64_t* __restrict__ out
) {
	__shared__ uint32_t s_scan[kWaves];
	uint64_t v[kUniqPer];
	const uint32_t flag = hash_occupied(table, slots, blockIdx.x * kUniqItems + threadIdx.x * kUniqPer, v);
	uint32_t c[1] = { static_cast<uint32_t>(__popc(flag)) }, tot[1];
	block_excl_add<1>(c, tot, s_scan);
	uint32_t o = blk_base[blockIdx.x] + c[0];
#pragma unroll
	for (uint32_t q = 0; q < kUniqPer; q++) if ((flag >> q) & 1u) out[o++] = v[q];
	if (blockIdx.x == 0 && threadIdx.x == 0 && *has_max) out[*n_found] = kLabelHashEmpty;
}

// The flat label section (labels.hpp:123-152) assembled on device:
//   u64 num_unique | uniq[num_unique] : stored_width | cc_per_slice[sz] : component_width | key[N] : byte_width(num_unique)
// grid = ceil(max(U, sz, N) / 256) over three index spaces handled by one kernel
__global__ void __launch_bounds__(kBlock) k_flat_section(
	const uint64_t* __restrict__ uniq, const uint32_t* __restrict__ n_uniq, int stored_width,
	const uint32_t* __restrict__ ncomp, uint32_t nslices, int component_width,
	const uint64_t* __restrict__ mapping, uint32_t n, uint8_t* __restrict__ out, uint32_t* __restrict__ missing
) {
	const uint32_t nu = *n_uniq;
	const int key_width = nu <= 0xFFu ? 1 : (nu <= 0xFFFFu ? 2 : 4);
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i == 0) for (int b = 0; b < 8; b++) out[b] = static_cast<uint8_t>((static_cast<uint64_t>(nu) >> (8 * b)) & 0xFF);
	uint8_t* o_uniq = out + 8;
	uint8_t* o_cc = o_uniq + static_cast<uint64_t>(nu) * stored_width;
	uint8_t* o_keys = o_cc + static_cast<uint64_t>(nslices) * component_width;
	if (i < nu) {
		const uint64_t v = uniq[i];
		for (int b = 0; b < stored_width; b++) o_uniq[static_cast<uint64_t>(i) * stored_width + b] = static_cast<uint8_t>((v >> (8 * b)) & 0xFF);
	}
	if (i < nslices) {
		const uint32_t v = ncomp[i];
		for (int b = 0; b < component_width; b++) o_cc[static_cast<uint64_t>(i) * component_width + b] = b < 4 ? static_cast<uint8_t>((v >> (8 * b)) & 0xFF) : 0;
	}
	if (i < n) {
		const uint64_t v = mapping[i];
		uint32_t lo = 0, hi = nu;          // last index with uniq[idx] <= v
		while (lo + 1 < hi) {
			const uint32_t mid = (lo + hi) >> 1;
			if (uniq[mid] <= v) lo = mid; else hi = mid;
		}
		if (missing && (nu == 0 || uniq[lo] != v)) *missing = 1u;      // a caller's list (merge_unique) without this label
		for (int b = 0; b < key_width; b++) o_keys[static_cast<uint64_t>(i) * key_width + b] = static_cast<uint8_t>((lo >> (8 * b)) & 0xFF);
	}
}

// ------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------

// geometric-sum table of ckl_runs.hpp (k_run_resolve), cached per slice size
void ensure_geom_table(ckl_encoder& e, uint64_t sxy) {
	LabelStage& ls = e.ls;
	if (ls.g_table_pixels == sxy && ls.d_G.p) return;
	hipStream_t s = e.stream2;
	const uint32_t npx = static_cast<uint32_t>(sxy);
	const uint32_t B = 1024, nblk = npx / B + 1;
	std::vector<uint32_t> g_base(B), blk_g(nblk), blk_x(nblk);
	const uint32_t X = gf_xpow(32);
	g_base[0] = 0;
	for (uint32_t i = 1; i < B; i++) g_base[i] = gf_mul(X, g_base[i - 1] ^ 0x80000000u);
	const uint32_t gB = gf_mul(X, g_base[B - 1] ^ 0x80000000u);
	const uint32_t XB = gf_xpow(32ull * B);
	blk_g[0] = 0; blk_x[0] = 0x80000000u;
	for (uint32_t k = 1; k < nblk; k++) {
		blk_g[k] = blk_g[k - 1] ^ gf_mul(blk_x[k - 1], gB);
		blk_x[k] = gf_mul(blk_x[k - 1], XB);
	}
	DevBuf<uint32_t> t_base, t_g, t_x;
	upload(t_base, g_base, s); upload(t_g, blk_g, s); upload(t_x, blk_x, s);
	ls.d_G.ensure(static_cast<size_t>(npx) + 1);
	hipLaunchKernelGGL(k_build_geom_table, dim3(npx / kBlock + 1), dim3(kBlock), 0, s, t_base.p, t_g.p, t_x.p, npx, ls.d_G.p);
	CKL_HIP(hipStreamSynchronize(s));
	ls.g_table_pixels = sxy;
}

// the run kernels' view of the session's run tables (ckl_runs.hpp)
RunArrays flat_arrays(const ckl_encoder& e) {
	const LabelStage& ls = e.ls;
	RunArrays ra;
	ra.word_base = ls.d_word_base.p; ra.rbase = ls.d_rbase.p; ra.rcap = ls.d_rcap.p;
	ra.parent = ls.d_parent.p; ra.run_start = ls.d_run_start.p; ra.run_cc = ls.d_run_cc.p;
	ra.nruns = ls.d_nruns.p; ra.ncomp = ls.d_ncomp.p; ra.slice_err = e.d_slice_err2.p;
	ra.comp_pix = ls.d_comp_pix.p;
	return ra;
}

// component counts, crc accumulators, id widths and error words of the slices lie side by side, the strip kernels' overflow
// word behind them: flat_collect brings them back in ONE transfer (four separate round trips cost the label path 0.2 ms,
// and it is what the encode ends with)
void flat_report_layout(ckl_encoder& e, uint32_t ns, hipStream_t s) {
	LabelStage& ls = e.ls;
	ls.d_flat_report.ensure(4 * static_cast<size_t>(ns) + 1);
	ls.d_ncomp.borrow(ls.d_flat_report.p, ns); ls.d_crc_acc.borrow(ls.d_flat_report.p + ns, ns);
	ls.d_idbits.borrow(ls.d_flat_report.p + 2 * static_cast<size_t>(ns), ns); e.d_slice_err2.borrow(ls.d_flat_report.p + 3 * static_cast<size_t>(ns), ns);
	CKL_HIP(hipMemsetAsync(e.d_slice_err2.p, 0, (static_cast<size_t>(ns) + 1) * sizeof(uint32_t), s));      // the error words and the overflow word
}

// the label planes as the run and strip kernels read them
RunGeom flat_geom(const ckl_encoder& e, int64_t sx, int64_t sy, uint32_t ns) {
	RunGeom g;
	g.planeV = plane_v(e); g.planeH = plane_h(e, ns);
	g.row_words = e.row_words; g.plane_words = e.plane_words;
	g.flip = 1u;   // a set bit (labels differ) is a break, whatever the stream's crack format
	g.sx = static_cast<uint32_t>(sx); g.sy = static_cast<uint32_t>(sy);
	return g;
}

// encode_flat per-slice part (labels.hpp:56-88) on runs of the label planes, the general pipeline of ckl_runs.hpp:
// components and their crc32c from one table entry per run.  It serves what the strip kernels below do not take.
void flat_enqueue_runs(ckl_encoder& e, int64_t sx, int64_t sy, int64_t sz) {
	LabelStage& ls = e.ls;
	hipStream_t s = e.stream2;
	const uint32_t ns = static_cast<uint32_t>(sz);
	const uint64_t sxy = static_cast<uint64_t>(sx) * sy;
	ls.flat_strips = false;

	// a run starts at x = 0 of every row and wherever the left neighbour differs
	// (the host tables stay alive in the session: nothing here waits for the uploads)
	std::vector<uint64_t>& rbase = ls.h_rbase;
	std::vector<uint32_t>& rcap = ls.h_rcap;
	rbase.assign(ns, 0); rcap.assign(ns, 0);
	uint64_t rtot = 0;
	uint32_t max_rcap = 0;
	for (uint32_t zi = 0; zi < ns; zi++) {
		const uint64_t runs = static_cast<uint64_t>(sy) + e.count_v[zi];
		rbase[zi] = rtot; rcap[zi] = static_cast<uint32_t>(runs); rtot += runs;
		max_rcap = std::max<uint32_t>(max_rcap, static_cast<uint32_t>(runs));
	}
	upload(ls.d_rbase, rbase, s); upload(ls.d_rcap, rcap, s);
	ls.d_word_base.ensure(e.plane_words * ns);
	ls.d_parent.ensure(rtot); ls.d_run_start.ensure(rtot); ls.d_run_cc.ensure(rtot); ls.d_comp_pix.ensure(rtot);
	ls.d_nruns.ensure(ns);
	flat_report_layout(e, ns, s);

	const RunGeom g = flat_geom(e, sx, sy, ns);
	const RunArrays ra = flat_arrays(e);
	hipLaunchKernelGGL(k_run_index, dim3(ns), dim3(kIndexBlock), 0, s, g, ra);
	launch_run_union(s, ns, g, ra);
	ResolveScratch rs;
	rs.nblk = (max_rcap + kBlock - 1) / kBlock;
	ls.d_run_local.ensure(rtot);
	ls.d_blk_roots.ensure(static_cast<size_t>(rs.nblk) * ns);
	rs.run_local = ls.d_run_local.p; rs.blk_roots = ls.d_blk_roots.p;
	launch_run_resolve(s, ns, ra, rs, ls.d_G.p, static_cast<uint32_t>(sxy), 0u, ls.d_crc_acc.p, ls.d_idbits.p);
	HT_MARK("f:enqueue_runs");
}

// k_slice_resolve_enc's table: the label stream runs beside two walks per CU and keeps to the 40 KiB that
// label_start (ckl_encode.hip) leaves it; a slice with more strip components gets a CU's LDS (flat_collect)
uint32_t flat_resolve_cap(size_t lds_bytes) {
	const char* env = getenv("CKL_ENC_RESOLVE_CAP");      // testing: forces the hand-over
	uint32_t cap = static_cast<uint32_t>(std::min<size_t>(kResolveCap, (lds_bytes - (kMaxStrips + 64u) * 4u) / 4u));
	if (env) cap = std::min<uint32_t>(cap, static_cast<uint32_t>(std::max(1, atoi(env))));
	return cap;
}
uint32_t flat_resolve_cap_max(ckl_encoder& e) {
	if (!e.ls.max_lds) CKL_HIP(hipDeviceGetAttribute(&e.ls.max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, e.device));
	return flat_resolve_cap(static_cast<size_t>(e.ls.max_lds) - 8192u);
}

// Can the strip kernels label this volume, and with what strips?  The host knows every slice's run count: the strips
// are sized from the densest slice, the decoder's rule (decoder_build) with the true density instead of an estimate
// and the encoder's table size (kEncStripCap).
// Not theirs: rows wider than a strip, more strips than the resolve takes, a densest slice of which not one row fits
// a strip, and a slice that must have more components than the largest resolve table holds (every component has a run
// that nothing joins to the row above: at least runs minus vertically equal pixel pairs) — noise pays nothing extra.
bool flat_strip_plan(ckl_encoder& e, int64_t sx, int64_t sy, uint32_t ns) {
	const bool runs_only = getenv("CKL_ENC_LABEL_RUNS") != nullptr;      // A/B and tests: the run pipeline for everything
	const char* cap_env = getenv("CKL_ENC_STRIP_CAP");                   // testing: strips overflow
	if (runs_only) return false;
	LabelStage& ls = e.ls;
	const uint64_t sxy = static_cast<uint64_t>(sx) * sy;
	if (e.row_words == 0 || e.row_words > kStripWords || sxy >= 0xFFFF0000ull) return false;
	uint64_t runs_max = 0, comps_min = 0;
	const uint64_t pairs_up = static_cast<uint64_t>(sx) * (sy - 1);
	for (uint32_t zi = 0; zi < ns; zi++) {
		const uint64_t runs = static_cast<uint64_t>(sy) + e.count_v[zi];
		const uint64_t equal_up = pairs_up - std::min<uint64_t>(pairs_up, e.count_h[zi]);
		runs_max = std::max<uint64_t>(runs_max, runs);
		comps_min = std::max<uint64_t>(comps_min, runs > equal_up ? runs - equal_up : 0ull);
	}
	const double runs_per_row = static_cast<double>(runs_max) / static_cast<double>(sy);
	const uint32_t fit = static_cast<uint32_t>(0.7 * kEncStripCap / runs_per_row);
	if (fit < 1u) return false;
	const uint32_t rows = std::max<uint32_t>(1u, std::min<uint32_t>(kStripWords / e.row_words, fit));
	const uint32_t nstrips = (static_cast<uint32_t>(sy) + rows - 1) / rows;
	if (nstrips > kMaxStrips || comps_min > flat_resolve_cap_max(e)) return false;
	ls.flat_strip_rows = rows; ls.flat_nstrips = nstrips;
	ls.flat_strip_cap = static_cast<uint32_t>(std::min<uint64_t>(kEncStripCap, static_cast<uint64_t>(rows) * sx));
	if (cap_env) ls.flat_strip_cap = std::min<uint32_t>(ls.flat_strip_cap, static_cast<uint32_t>(std::max(1, atoi(cap_env))));
	return true;
}

StripArrays flat_strip_arrays(const ckl_encoder& e) {
	const LabelStage& ls = e.ls;
	StripArrays sa = {};
	sa.run_lid = ls.s_run_lid.p; sa.sc_w = ls.s_sc_w.p; sa.sc_cc = ls.s_sc_first.p;
	sa.strip_nruns = ls.s_strip_nruns.p; sa.strip_nsc = ls.s_strip_nsc.p;
	sa.seam_first = ls.s_seam_first.p; sa.seam_last = ls.s_seam_last.p;
	sa.slice_err = e.d_slice_err2.p; sa.overflow = ls.d_flat_report.p + 4 * ls.d_ncomp.n;
	sa.nstrips = ls.flat_nstrips; sa.strip_rows = ls.flat_strip_rows; sa.cap = ls.flat_strip_cap; sa.zbase = 0;
	return sa;
}

// k_slice_resolve_enc over all slices with a table of `cap` entries
void flat_launch_resolve(ckl_encoder& e, const void* labels, int64_t sx, int64_t sy, uint32_t ns, uint32_t cap) {
	LabelStage& ls = e.ls;
	hipStream_t s = e.stream2;
	ls.flat_resolve_cap = cap;
	ls.d_label_slots.ensure(static_cast<size_t>(ns) * cap);
	ResolveArgs ra = {};
	ra.cap = cap;
	EncResolve en;
	en.labels = labels; en.sxy = static_cast<uint64_t>(sx) * sy; en.slots = ls.d_label_slots.p; en.crc_acc = ls.d_crc_acc.p; en.idbits = ls.d_idbits.p;
	const RunGeom g = flat_geom(e, sx, sy, ns);
	const StripArrays sa = flat_strip_arrays(e);
	const size_t tab_bytes = static_cast<size_t>(cap) * sizeof(uint32_t);
	if (e.label_src) {
		// no volume: the slots receive the components' first pixels, flat_collect turns them into labels
		allow_dynamic_lds(reinterpret_cast<const void*>(&k_slice_resolve_enc_pixels), e.device, tab_bytes);
		hipLaunchKernelGGL(k_slice_resolve_enc_pixels, dim3(ns), dim3(kResolveBlock), tab_bytes, s, g, sa, ra, en, ls.d_ncomp.p);
		return;
	}
	with_label_type(e.dtype_bytes, [&](auto t) {
		typedef typename decltype(t)::type LABEL;
		allow_dynamic_lds(reinterpret_cast<const void*>(&k_slice_resolve_enc<LABEL>), e.device, tab_bytes);
		hipLaunchKernelGGL(k_slice_resolve_enc<LABEL>, dim3(ns), dim3(kResolveBlock), tab_bytes, s, g, sa, ra, en, ls.d_ncomp.p);
	});
}

}  // namespace

// (what the stage is and what need_runs / beside_walk mean: ckl_encode_labels.hpp)
void ckl::flat_enqueue(ckl_encoder& e, const void* labels, int64_t sx, int64_t sy, int64_t sz, bool need_runs, bool beside_walk) {
	LabelStage& ls = e.ls;
	hipStream_t s = e.stream2;
	const uint32_t ns = static_cast<uint32_t>(sz);
	const uint64_t sxy = static_cast<uint64_t>(sx) * sy;
	ensure_geom_table(e, sxy);
	if (need_runs || !beside_walk || !flat_strip_plan(e, sx, sy, ns)) { flat_enqueue_runs(e, sx, sy, sz); return; }
	ls.flat_strips = true;
	const size_t nst = static_cast<size_t>(ls.flat_nstrips) * ns;
	ls.s_strip_nruns.ensure(nst); ls.s_strip_nsc.ensure(nst);
	ls.s_seam_first.ensure(nst * e.row_words); ls.s_seam_last.ensure(nst * e.row_words);
	ls.s_run_lid.ensure(nst * ls.flat_strip_cap); ls.s_sc_w.ensure(nst * ls.flat_strip_cap); ls.s_sc_first.ensure(nst * ls.flat_strip_cap);
	flat_report_layout(e, ns, s);
	hipLaunchKernelGGL(k_strip_ccl_enc, dim3(ls.flat_nstrips, ns), dim3(kBlock), 0, s, flat_geom(e, sx, sy, ns), flat_strip_arrays(e), ls.d_G.p, static_cast<uint32_t>(sxy));
	flat_launch_resolve(e, labels, sx, sy, ns, flat_resolve_cap(kFlatResolveLds));
	HT_MARK("f:enqueue_strips");
}

void ckl::flat_collect(ckl_encoder& e, const void* labels, int label_width, int64_t sx, int64_t sy, int64_t sz, FlatResult& out) {
	LabelStage& ls = e.ls;
	hipStream_t s = e.stream2;
	const uint32_t ns = static_cast<uint32_t>(sz);
	const uint64_t sxy = static_cast<uint64_t>(sx) * sy;
	// laid out by flat_report_layout: ncomp | crc_acc | idbits | slice_err2 | overflow, one transfer
	const size_t rep_n = 4 * static_cast<size_t>(ns) + 1;
	std::vector<uint32_t> rep = download(ls.d_flat_report.p, rep_n, s);
	if (ls.flat_strips && rep[rep_n - 1] == 2u && ls.flat_resolve_cap < flat_resolve_cap_max(e)) {
		// only k_slice_resolve_enc's table was too small, and it can be larger (over-segmented slices): once more with a
		// CU's LDS per slice, as the decoder does; the strips' tables stand
		CKL_HIP(hipMemsetAsync(ls.d_flat_report.p + rep_n - 1, 0, sizeof(uint32_t), s));
		flat_launch_resolve(e, labels, sx, sy, ns, flat_resolve_cap_max(e));
		HT_MARK("f:resolve_retry");
		rep = download(ls.d_flat_report.p, rep_n, s);
	}
	if (ls.flat_strips && rep[rep_n - 1]) {
		// a strip or a resolve table overflowed: the whole volume again on the run pipeline
		flat_enqueue_runs(e, sx, sy, sz);
		rep = download(ls.d_flat_report.p, rep_n, s);
	}
	const uint32_t *acc = rep.data() + ns, *idbits = rep.data() + 2 * static_cast<size_t>(ns), *errs = rep.data() + 3 * static_cast<size_t>(ns);
	out.ncomp.assign(rep.begin(), rep.begin() + ns);
	HT_MARK(ls.flat_strips ? "f:wait_strips" : "f:wait_runs");
	for (uint32_t zi = 0; zi < ns; zi++) if (errs[zi]) throw Error(CKL_ERR_RUNTIME, "crackle_amd: run table overflow on z=" + std::to_string(zi));
	const uint32_t init_term = gf_mul(0xFFFFFFFFu, gf_xpow(32ull * sxy));
	out.crcs.resize(ns);
	uint32_t fix_bits = 0xFFFFFFFFu, fix = 0;
	for (uint32_t zi = 0; zi < ns; zi++) {
		if (idbits[zi] != fix_bits) { fix_bits = idbits[zi]; fix = gf_xpow(32 - fix_bits); }
		out.crcs[zi] = ~(gf_mul(acc[zi], fix) ^ init_term);
	}

	// (the offsets stay alive in the session: nothing here waits for their upload)
	std::vector<uint64_t>& comp_off = ls.h_comp_off;
	comp_off.assign(ns, 0);
	uint64_t total = 0;
	for (uint32_t zi = 0; zi < ns; zi++) { comp_off[zi] = total; total += out.ncomp[zi]; }
	upload(ls.d_comp_off, comp_off, s);
	e.d_mapping.ensure(total + 1);
	uint32_t max_ncomp = 1;
	for (uint32_t zi = 0; zi < ns; zi++) max_ncomp = std::max(max_ncomp, out.ncomp[zi]);
	const dim3 grid((max_ncomp + kBlock - 1) / kBlock, ns);
	if (e.label_src) hipLaunchKernelGGL(k_component_labels_from_runs, grid, dim3(kBlock), 0, s, *e.label_src,
		ls.flat_strips ? ls.d_label_slots.p : nullptr, ls.flat_resolve_cap, ls.d_comp_pix.p, ls.d_rbase.p, ls.d_ncomp.p, ls.d_comp_off.p, e.d_mapping.p);
	else if (ls.flat_strips) hipLaunchKernelGGL(k_gather_slots, grid, dim3(kBlock), 0, s, ls.d_label_slots.p, ls.flat_resolve_cap, ls.d_ncomp.p, ls.d_comp_off.p, e.d_mapping.p);
	else with_label_type(label_width, [&](auto t) {
		typedef typename decltype(t)::type LABEL;
		hipLaunchKernelGGL(k_mapping_comps<LABEL>, grid, dim3(kBlock), 0, s, static_cast<const LABEL*>(labels), flat_arrays(e), sxy, ls.d_comp_off.p, e.d_mapping.p);
	});
	out.total = total;
}

uint64_t ckl::flat_section(ckl_encoder& e, uint64_t N, int stored_width, int component_width, uint32_t ns, const ckl_encode_overrides* ov) {
	const bool sort_all = getenv("CKL_LABEL_SORT_ALL") != nullptr;
	const bool single_steps = getenv("CKL_BITONIC_SINGLE_STEPS") != nullptr;
	LabelStage& ls = e.ls;
	hipStream_t s = e.stream2;
	if (N > 0x7FFFFFFFull) throw Error(CKL_ERR_RUNTIME, "crackle_amd: too many components");
	ls.d_n_uniq.ensure(2);
	ls.d_uniq.ensure(N + 1);
	// the values to sort: the distinct labels when the components are many (a hash pass, then the
	// sort network runs over tens of thousands instead of millions of keys), else all of them
	const uint64_t* sort_src = e.d_mapping.p;
	uint64_t n_sort = N;
	if (N > 8192 && N <= (1ull << 26) && !sort_all) {
		uint32_t slots = 16384;
		while (slots < 2 * N) slots <<= 1;
		ls.d_label_hash.ensure(slots);
		CKL_HIP(hipMemsetAsync(ls.d_label_hash.p, 0xFF, static_cast<size_t>(slots) * sizeof(uint64_t), s));
		CKL_HIP(hipMemsetAsync(ls.d_n_uniq.p, 0, 2 * sizeof(uint32_t), s));
		unsigned long long* table = reinterpret_cast<unsigned long long*>(ls.d_label_hash.p);
		hipLaunchKernelGGL(k_label_hash_insert, dim3(static_cast<uint32_t>((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, e.d_mapping.p, static_cast<uint32_t>(N), table, slots - 1u, ls.d_n_uniq.p + 1);
		const uint32_t hb = (slots + kUniqItems - 1) / kUniqItems;
		ls.d_uniq_blk.ensure(hb + 1);
		hipLaunchKernelGGL(k_label_hash_count, dim3(hb), dim3(kBlock), 0, s, table, slots, ls.d_uniq_blk.p);
		hipLaunchKernelGGL(k_unique_scan, dim3(1), dim3(kBlock), 0, s, ls.d_uniq_blk.p, hb, ls.d_n_uniq.p);
		hipLaunchKernelGGL(k_label_hash_scatter, dim3(hb), dim3(kBlock), 0, s, table, slots, ls.d_uniq_blk.p, ls.d_n_uniq.p, ls.d_n_uniq.p + 1, ls.d_uniq.p);
		const std::vector<uint32_t> found = download(ls.d_n_uniq.p, 2, s);
		n_sort = static_cast<uint64_t>(found[0]) + (found[1] ? 1u : 0u);
		if (n_sort == 0 || n_sort > N) throw Error(CKL_ERR_RUNTIME, "crackle_amd: label table pass failed");
		ls.d_label_list.ensure(n_sort);
		CKL_HIP(hipMemcpyAsync(ls.d_label_list.p, ls.d_uniq.p, n_sort * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
		sort_src = ls.d_label_list.p;
	}
	// sharded encode: the ranks' lists are merged (and sorted) by the caller anyway, so the slab's distinct
	// labels go out as the hash pass left them and the local sort is skipped
	const bool merge_unsorted = ov && ov->merge_unique && sort_src == ls.d_label_list.p;
	uint32_t n_pad = 2048;
	while (n_pad < n_sort) n_pad <<= 1;
	if (!merge_unsorted) {
	ls.d_sorted.ensure(n_pad);
	const uint32_t blocks = (n_pad + kBlock - 1) / kBlock;
	hipLaunchKernelGGL(k_pad_copy_u64, dim3(blocks), dim3(kBlock), 0, s, sort_src, n_sort, ls.d_sorted.p, static_cast<uint64_t>(n_pad));
	hipLaunchKernelGGL(k_bitonic_first, dim3(n_pad / 2048), dim3(kBlock), 0, s, ls.d_sorted.p, n_pad);
	for (uint32_t k = 4096; k <= n_pad; k <<= 1) {
		uint32_t j = k >> 1;
		for (; j >= 4096 && !single_steps; j >>= 2) hipLaunchKernelGGL(k_bitonic_step2, dim3((n_pad / 4 + kBlock - 1) / kBlock), dim3(kBlock), 0, s, ls.d_sorted.p, j, k, n_pad);
		for (; j >= 2048; j >>= 1) hipLaunchKernelGGL(k_bitonic_step, dim3(blocks), dim3(kBlock), 0, s, ls.d_sorted.p, j, k, n_pad);
		hipLaunchKernelGGL(k_bitonic_local, dim3(n_pad / 2048), dim3(kBlock), 0, s, ls.d_sorted.p, j, k, n_pad);
	}
	{
		const uint32_t ub = static_cast<uint32_t>((n_sort + kUniqItems - 1) / kUniqItems);
		ls.d_uniq_blk.ensure(ub + 1);
		hipLaunchKernelGGL(k_unique_count, dim3(ub), dim3(kBlock), 0, s, ls.d_sorted.p, static_cast<uint32_t>(n_sort), ls.d_uniq_blk.p);
		hipLaunchKernelGGL(k_unique_scan, dim3(1), dim3(kBlock), 0, s, ls.d_uniq_blk.p, ub, ls.d_n_uniq.p);
		hipLaunchKernelGGL(k_unique_scatter, dim3(ub), dim3(kBlock), 0, s, ls.d_sorted.p, static_cast<uint32_t>(n_sort), ls.d_uniq_blk.p, ls.d_uniq.p);
	}
	}
	uint64_t uniq_bound = N;      // entries of the unique list the section kernel may have to write
	const bool merged_list = ov && ov->merge_unique;
	if (ov && ov->merge_unique) {
		// sharded encode: the keys are written against the unique labels of all slabs.  The caller
		// exchanges the lists now, under the crack trail that is still running on the other stream.
		HT_MARK("l:enqueue");
		const uint32_t n_local = merge_unsorted ? static_cast<uint32_t>(n_sort) : download(ls.d_n_uniq.p, 1, s)[0];
		std::vector<uint64_t> local = download(merge_unsorted ? ls.d_label_list.p : ls.d_uniq.p, n_local, s);      // distinct; sorted unless merge_unsorted
		HT_MARK("l:local");
		const uint64_t* merged = nullptr;
		uint64_t n_merged = 0;
		if (ov->merge_unique(ov->merge_ctx, local.data(), n_local, &merged, &n_merged) != 0 || (!merged && n_merged))
			throw Error(CKL_ERR_RUNTIME, "crackle_amd: the merge_unique callback failed");
		HT_MARK("l:merge");
		if (n_merged < n_local || n_merged > 0xFFFFFFFFull) throw Error(CKL_ERR_ARG, "crackle_amd: merge_unique returned a list that cannot contain the slab's labels");
		ls.d_uniq.ensure(n_merged + 1);
		if (n_merged) CKL_HIP(hipMemcpyAsync(ls.d_uniq.p, merged, n_merged * sizeof(uint64_t), hipMemcpyHostToDevice, s));
		const uint32_t nm[2] = { static_cast<uint32_t>(n_merged), 0u };      // the list's length and the section kernel's "label not in the list"
		CKL_HIP(hipMemcpyAsync(ls.d_n_uniq.p, nm, sizeof(nm), hipMemcpyHostToDevice, s));
		CKL_HIP(hipStreamSynchronize(s));      // `nm` and the caller's list may go away
		e.d_labels_bin.ensure(8 + n_merged * static_cast<uint64_t>(stored_width) + static_cast<uint64_t>(ns) * component_width + N * 4 + 16);
		uniq_bound = std::max<uint64_t>(uniq_bound, n_merged);
	}
	// worst case: every component has its own label and 4-byte keys
	e.d_labels_bin.ensure(8 + N * static_cast<uint64_t>(stored_width) + static_cast<uint64_t>(ns) * component_width + N * 4 + 16);
	const uint64_t work = std::max<uint64_t>(std::max<uint64_t>(uniq_bound, ns), 1);
	hipLaunchKernelGGL(k_flat_section, dim3(static_cast<uint32_t>((work + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
		ls.d_uniq.p, ls.d_n_uniq.p, stored_width, ls.d_ncomp.p, ns, component_width, e.d_mapping.p, static_cast<uint32_t>(N), e.d_labels_bin.p,
		merged_list ? ls.d_n_uniq.p + 1 : nullptr);
	HT_MARK("l:enqueue");
	const std::vector<uint32_t> report = download(ls.d_n_uniq.p, merged_list ? 2 : 1, s);
	const uint32_t nu = report[0];
	HT_MARK("l:wait");
	// the length alone does not show it: keys against a list without one of the slab's labels (or one that is not sorted) would name its neighbour
	if (merged_list && report[1]) throw Error(CKL_ERR_ARG, "crackle_amd: merge_unique returned a list that lacks a label of the slab");
	return 8 + static_cast<uint64_t>(nu) * stored_width + static_cast<uint64_t>(ns) * component_width + N * static_cast<uint64_t>(byte_width(nu));
}

void ckl::paint_components(ckl_encoder& e, int64_t sx, int64_t sy, int64_t sz, uint32_t id_base, uint32_t* cc_device) {
	const LabelStage& ls = e.ls;
	launch_paint_components(e.stream2, plane_v(e), e.row_words, e.plane_words, sx, sy, sz, ls.d_word_base.p, ls.d_rbase.p, ls.d_run_cc.p, ls.d_comp_off.p, id_base, cc_device);
}
