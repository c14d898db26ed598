// Operations on a decoded stream: label statistics, contacts, overlaps, connected components
// (ckl_components3d.hpp), the point cloud (ckl_contours.hpp), the voxel connectivity graph,
// array_equal and mode_pooling_2x2x1.  Each is here whole (kernels, host driver, C entry point) and
// consumes what a decode session (ckl_decoder.hpp) leaves in HBM after decoder_run reached the goal
// the operation asks for.
#include "ckl_decoder.hpp"
#include "ckl_contours.hpp"

#include <algorithm>
#include <chrono>
#include <deque>
#include <memory>

namespace ckl {

using namespace dev;

// ------------------------------------------------------------------------------
// per-label statistics over the runs (operations.hpp:321-618: voxel_counts, centroids,
// bounding_boxes).  The reference walks every pixel of the slice's component image into
// per-component accumulators and merges those into the per-label maps through label_map.
// A run is a stretch of one row, so its voxel count, coordinate sums and x extent are closed
// forms of its end points: one workgroup per slice adds its runs into per-component
// accumulators in LDS, then merges the components into the label table (a binary search per
// component) with global atomics.  A slice with more components than the LDS holds merges
// run by run instead.
// ------------------------------------------------------------------------------
constexpr int kStatsBlock = 1024;
constexpr uint32_t kStatsBytesPerComp = 8 + 8 + 4 * 5;   // sum x, sum y, N, xmin, xmax, ymin, ymax

__device__ __forceinline__ uint32_t stats_find(const StatsArgs& sa, uint64_t v) {
	uint32_t lo = 0, hi = sa.n_table;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (sa.table[mid] < v) lo = mid + 1; else hi = mid;
	}
	return (lo < sa.n_table && sa.table[lo] == v) ? lo : 0xFFFFFFFFu;
}

__device__ __forceinline__ void stats_merge(
	const StatsArgs& sa, uint32_t idx, uint32_t z, unsigned long long n, unsigned long long sumx, unsigned long long sumy,
	uint32_t xmin, uint32_t xmax, uint32_t ymin, uint32_t ymax
) {
	unsigned long long* acc = sa.acc + 4ull * idx;
	atomicAdd(acc + 0, n); atomicAdd(acc + 1, sumx); atomicAdd(acc + 2, sumy); atomicAdd(acc + 3, n * z);
	uint32_t* box = sa.box + 6ull * idx;
	atomicMin(box + 0, xmin); atomicMin(box + 1, ymin); atomicMin(box + 2, z);
	atomicMax(box + 3, xmax); atomicMax(box + 4, ymax); atomicMax(box + 5, z);
}

// grid = nslices, block = kStatsBlock, dynamic LDS = lds_comps * kStatsBytesPerComp
static __global__ void __launch_bounds__(kStatsBlock) k_run_stats(
	RunArrays r, const uint64_t* __restrict__ label_map, const uint64_t* __restrict__ comp_off,
	const uint32_t* __restrict__ ncomp_expect, StatsArgs sa
) {
	extern __shared__ __attribute__((aligned(16))) unsigned char s_stats[];
	const uint32_t zi = blockIdx.x;
	const uint32_t z = sa.z_start + zi;
	const uint32_t n = r.nruns[zi];
	const uint32_t nc = ncomp_expect[zi];
	const uint64_t rb = r.rbase[zi];
	const uint64_t* lmap = label_map + comp_off[zi];
	const bool in_lds = nc <= sa.lds_comps;
	const uint32_t cap = sa.lds_comps;
	unsigned long long* s_sumx = reinterpret_cast<unsigned long long*>(s_stats);
	unsigned long long* s_sumy = s_sumx + cap;
	uint32_t* s_n = reinterpret_cast<uint32_t*>(s_sumy + cap);
	uint32_t* s_xmin = s_n + cap;
	uint32_t* s_xmax = s_xmin + cap;
	uint32_t* s_ymin = s_xmax + cap;
	uint32_t* s_ymax = s_ymin + cap;
	if (in_lds) {
		for (uint32_t c = threadIdx.x; c < nc; c += kStatsBlock) {
			s_sumx[c] = 0; s_sumy[c] = 0; s_n[c] = 0;
			s_xmin[c] = 0xFFFFFFFFu; s_xmax[c] = 0; s_ymin[c] = 0xFFFFFFFFu; s_ymax[c] = 0;
		}
		__syncthreads();
	}
	for (uint32_t i = threadIdx.x; i < n; i += kStatsBlock) {
		const uint32_t a = r.run_start[rb + i];
		const uint32_t b = (i + 1 < n) ? r.run_start[rb + i + 1] : sa.n_pixels;
		const uint32_t cc = r.run_cc[rb + i];
		if (b <= a) continue;
		if (cc >= nc) { atomicOr(r.slice_err + zi, ERR_NCOMP); continue; }
		const uint32_t y = a / sa.sx;
		const uint32_t x0 = a - y * sa.sx;
		const uint32_t len = b - a;
		const uint32_t x1 = x0 + len - 1;
		const unsigned long long sumx = (static_cast<unsigned long long>(x0) + x1) * len / 2;
		const unsigned long long sumy = static_cast<unsigned long long>(y) * len;
		if (in_lds) {
			atomicAdd(s_sumx + cc, sumx); atomicAdd(s_sumy + cc, sumy); atomicAdd(s_n + cc, len);
			atomicMin(s_xmin + cc, x0); atomicMax(s_xmax + cc, x1);
			atomicMin(s_ymin + cc, y); atomicMax(s_ymax + cc, y);
		}
		else {
			const uint32_t idx = stats_find(sa, lmap[cc]);
			if (idx == 0xFFFFFFFFu) { atomicOr(r.slice_err + zi, ERR_NCOMP); continue; }   // a label outside the table: inconsistent label section
			stats_merge(sa, idx, z, len, sumx, sumy, x0, x1, y, y);
		}
	}
	if (!in_lds) return;
	__syncthreads();
	for (uint32_t c = threadIdx.x; c < nc; c += kStatsBlock) {
		if (!s_n[c]) continue;
		const uint32_t idx = stats_find(sa, lmap[c]);
		if (idx == 0xFFFFFFFFu) { atomicOr(r.slice_err + zi, ERR_NCOMP); continue; }
		stats_merge(sa, idx, z, s_n[c], s_sumx[c], s_sumy[c], s_xmin[c], s_xmax[c], s_ymin[c], s_ymax[c]);
	}
}

static __global__ void k_stats_init(uint32_t* box, uint32_t n_table) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_table) return;
	box[6ull * i + 0] = box[6ull * i + 1] = box[6ull * i + 2] = 0xFFFFFFFFu;
	box[6ull * i + 3] = box[6ull * i + 4] = box[6ull * i + 5] = 0;
}

void launch_run_stats(ckl_decoder& d, const RunArrays& ra, const StatsArgs& sa) {
	hipLaunchKernelGGL(k_run_stats, dim3(d.nslices), dim3(kStatsBlock), static_cast<size_t>(sa.lds_comps) * kStatsBytesPerComp, d.stream,
		ra, d.d_label_map.p, d.d_comp_off.p, d.d_ncomp_expect.p, sa);
}

// ------------------------------------------------------------------------------
// contacts (operations.hpp:850-1021): faces between touching labels, counted per axis from the
// runs.  The reference walks every pixel of two consecutive component images and adds a float
// per face into a hash map.  Here a thread takes one run of a slice and counts
//   x  the boundary to the next run of its row, when the two components differ (one face);
//   y  the overlaps with the runs of the row above in the same slice whose component differs;
//   z  the overlaps with the runs of the same row in the previous slice of the range whose label
//      differs (only for z > z_start, as the reference).
// The run of the other row that holds the run's first pixel is found in O(1) through word_base
// and the vertical-crack plane (as k_label_map_pins does); the following runs of that row are
// walked until the run's last pixel.  Labels are indices into the sorted label table
// (k_component_label_index), a pair is the 64-bit key (min << 32 | max).  Exact integer counts:
// per workgroup in an LDS open-addressing table, flushed into a global one with 64-bit counters.
// A key that finds no room in the LDS table goes to the global table directly; a global table
// that fills sets a flag and the host runs the pass again with twice the capacity.
// ------------------------------------------------------------------------------
constexpr int kContactBlock = 256;
constexpr uint32_t kContactPer = 8;                                 // runs per thread
constexpr uint32_t kContactRuns = kContactBlock * kContactPer;      // runs per workgroup
constexpr uint32_t kContactLds = 1024;                              // LDS table entries (power of two)
constexpr uint32_t kContactProbes = 32;                             // LDS probes before a key goes to the global table
constexpr uint32_t kContactGlobalProbes = 128;                      // global probes before the table counts as full
constexpr unsigned long long kContactEmpty = ~0ull;                 // never a key: table indices are below 2^32 - 1
constexpr uint32_t kNoKey = 0xFFFFFFFFu;
enum : uint32_t { CONTACT_FULL = 0, CONTACT_BADKEY = 1, CONTACT_COUNT = 2, CONTACT_FLAGS = 3 };

struct ContactArgs {
	const uint32_t* comp_key;        // [total_comp] label table index of every component (kNoKey: not in the table)
	uint32_t zero_key;               // table index of label 0 (kNoKey: absent); its faces are dropped
	uint32_t sx, n_pixels;
	unsigned long long* keys;        // [cap] global table: pair keys, kContactEmpty where free
	unsigned long long* counts;      // [cap][3] faces along x, y, z
	uint32_t cap_mask;               // cap - 1, cap a power of two
	uint32_t* flags;                 // [CONTACT_FLAGS]: full, a label outside the table, compacted entries
};

__device__ __forceinline__ uint32_t contact_hash(unsigned long long k) {
	k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
	k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
	k ^= k >> 33;
	return static_cast<uint32_t>(k);
}

// The table is full for a key that finds neither itself nor a free entry in kContactGlobalProbes
// entries from its hash; a full table gives up at once (the pass runs again, twice as large).  No
// count of the entries taken: one word that every new key adds to serialises the kernel.
__device__ void contact_global(const ContactArgs& ca, unsigned long long key, uint32_t nx, uint32_t ny, uint32_t nz) {
	if (__hip_atomic_load(ca.flags + CONTACT_FULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
	const uint32_t h = contact_hash(key);
	for (uint32_t p = 0; p < kContactGlobalProbes && p <= ca.cap_mask; p++) {
		const uint32_t slot = (h + p) & ca.cap_mask;
		unsigned long long cur = ca.keys[slot];      // a slot changes once, from empty to its key: a stale read is settled by the CAS
		if (cur == kContactEmpty) {
			cur = atomicCAS(ca.keys + slot, kContactEmpty, key);
			if (cur == kContactEmpty) cur = key;
		}
		if (cur == key) {
			unsigned long long* c = ca.counts + 3ull * slot;
			if (nx) atomicAdd(c + 0, static_cast<unsigned long long>(nx));
			if (ny) atomicAdd(c + 1, static_cast<unsigned long long>(ny));
			if (nz) atomicAdd(c + 2, static_cast<unsigned long long>(nz));
			return;
		}
	}
	atomicOr(ca.flags + CONTACT_FULL, 1u);
}

// n faces along `axis` between the labels of table indices ka and kb
__device__ __forceinline__ void contact_add(
	const ContactArgs& ca, unsigned long long* s_key, uint32_t* s_cnt, uint32_t ka, uint32_t kb, uint32_t axis, uint32_t n
) {
	if (ka == ca.zero_key || kb == ca.zero_key) return;
	const unsigned long long key = ka <= kb ? (static_cast<unsigned long long>(ka) << 32 | kb) : (static_cast<unsigned long long>(kb) << 32 | ka);
	const uint32_t h = contact_hash(key);
	for (uint32_t p = 0; p < kContactProbes; p++) {
		const uint32_t slot = (h + p) & (kContactLds - 1);
		unsigned long long cur = s_key[slot];
		if (cur == kContactEmpty) {
			cur = atomicCAS(s_key + slot, kContactEmpty, key);
			if (cur == kContactEmpty) cur = key;
		}
		if (cur == key) { atomicAdd(s_cnt + 3 * slot + axis, n); return; }
	}
	contact_global(ca, key, axis == 0 ? n : 0u, axis == 1 ? n : 0u, axis == 2 ? n : 0u);
}

// faces between pixels [x0, x1] of a run (component cc, label index ka) and the runs of row y of
// slice zj: by component (y faces, same slice) or by label (z faces, previous slice)
__device__ __forceinline__ void contact_row(
	const RunGeom& g, const RunArrays& r, const ContactArgs& ca, unsigned long long* s_key, uint32_t* s_cnt,
	uint32_t zj, const uint32_t* key_j, uint32_t nce_j, uint32_t y, uint32_t x0, uint32_t x1, uint32_t cc, uint32_t ka, bool by_comp, uint32_t axis
) {
	const uint64_t rb = r.rbase[zj];
	const uint32_t nj = r.nruns[zj];
	const uint32_t row = y * ca.sx;
	const uint32_t w = x0 >> 5;
	uint32_t j = r.word_base[zj * g.plane_words + y * g.row_words + w] + __popc(g.breaks(zj, y, w) & mask_le(x0 & 31u)) - 1u;
	if (j >= nj) { atomicOr(ca.flags + CONTACT_BADKEY, 1u); return; }
	uint32_t s = r.run_start[rb + j] - row;
	for (;;) {
		// the run after the last one of a row starts the next row (or the slice ends): e <= sx
		const uint32_t e = (j + 1 < nj ? r.run_start[rb + j + 1] : ca.n_pixels) - row;
		const uint32_t ccj = r.run_cc[rb + j];
		if (!by_comp || ccj != cc) {
			const uint32_t kj = ccj < nce_j ? key_j[ccj] : kNoKey;
			if (kj == kNoKey) atomicOr(ca.flags + CONTACT_BADKEY, 1u);
			else if (by_comp || kj != ka) contact_add(ca, s_key, s_cnt, ka, kj, axis, min(e, x1 + 1) - max(s, x0));
		}
		if (e > x1) return;
		j++;
		s = e;
	}
}

// grid = (ceil(most runs of a slice / kContactRuns), nslices), block = kContactBlock
static __global__ void __launch_bounds__(kContactBlock) k_run_contacts(
	RunGeom g, RunArrays r, const uint64_t* __restrict__ comp_off, const uint32_t* __restrict__ ncomp_expect, ContactArgs ca
) {
	__shared__ unsigned long long s_key[kContactLds];
	__shared__ uint32_t s_cnt[3 * kContactLds];
	__shared__ uint32_t s_stop;
	const uint32_t zi = blockIdx.y;
	const uint32_t n = r.nruns[zi];
	const uint32_t i0 = blockIdx.x * kContactRuns;
	if (i0 >= n) return;
	if (threadIdx.x == 0) s_stop = __hip_atomic_load(ca.flags + CONTACT_FULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	for (uint32_t k = threadIdx.x; k < kContactLds; k += kContactBlock) {
		s_key[k] = kContactEmpty;
		s_cnt[3 * k] = 0; s_cnt[3 * k + 1] = 0; s_cnt[3 * k + 2] = 0;
	}
	__syncthreads();
	if (s_stop) return;      // this pass runs again with a larger table: nothing it adds is kept
	const uint64_t rb = r.rbase[zi];
	const uint32_t nce = ncomp_expect[zi];
	const uint32_t* key_z = ca.comp_key + comp_off[zi];
	const uint32_t nce_p = zi ? ncomp_expect[zi - 1] : 0u;
	const uint32_t* key_p = zi ? ca.comp_key + comp_off[zi - 1] : nullptr;
	for (uint32_t k = 0; k < kContactPer; k++) {
		const uint32_t i = i0 + k * kContactBlock + threadIdx.x;
		if (i >= n) break;
		const uint32_t a = r.run_start[rb + i];
		const uint32_t b = i + 1 < n ? r.run_start[rb + i + 1] : ca.n_pixels;
		const uint32_t cc = r.run_cc[rb + i];
		const uint32_t y = a / ca.sx;
		const uint32_t row = y * ca.sx;
		const uint32_t x0 = a - row, x1 = b - 1 - row;
		const uint32_t ka = cc < nce ? key_z[cc] : kNoKey;
		if (ka == kNoKey) { atomicOr(ca.flags + CONTACT_BADKEY, 1u); continue; }
		if (b < row + ca.sx) {      // the next run is in the same row
			const uint32_t cc2 = r.run_cc[rb + i + 1];
			if (cc2 != cc) {
				const uint32_t kb = cc2 < nce ? key_z[cc2] : kNoKey;
				if (kb == kNoKey) atomicOr(ca.flags + CONTACT_BADKEY, 1u);
				else contact_add(ca, s_key, s_cnt, ka, kb, 0, 1);
			}
		}
		if (y > 0) contact_row(g, r, ca, s_key, s_cnt, zi, key_z, nce, y - 1, x0, x1, cc, ka, true, 1);
		if (zi > 0) contact_row(g, r, ca, s_key, s_cnt, zi - 1, key_p, nce_p, y, x0, x1, cc, ka, false, 2);
	}
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < kContactLds; k += kContactBlock) {
		const unsigned long long key = s_key[k];
		if (key != kContactEmpty) contact_global(ca, key, s_cnt[3 * k], s_cnt[3 * k + 1], s_cnt[3 * k + 2]);
	}
}

// the occupied entries of the global table, packed (in no particular order: the host sorts them);
// one output offset per workgroup of kContactCompact entries.  NC counters per entry: 3 for
// contacts, 1 for overlaps.
constexpr uint32_t kContactCompactPer = 8;
constexpr uint32_t kContactCompact = kBlock * kContactCompactPer;
template <uint32_t NC>
static __global__ void __launch_bounds__(kBlock) k_contacts_compact(
	const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ counts, uint32_t cap,
	unsigned long long* __restrict__ out_keys, unsigned long long* __restrict__ out_counts, uint32_t* flags
) {
	__shared__ uint32_t s_scan[kWaves];
	__shared__ uint32_t s_base;
	const uint32_t i0 = blockIdx.x * kContactCompact + threadIdx.x * kContactCompactPer;
	unsigned long long k[kContactCompactPer];
	uint32_t v[1] = { 0 }, total[1];
#pragma unroll
	for (uint32_t j = 0; j < kContactCompactPer; j++) {
		k[j] = i0 + j < cap ? keys[i0 + j] : kContactEmpty;
		v[0] += k[j] != kContactEmpty;
	}
	block_excl_add<1>(v, total, s_scan);
	if (threadIdx.x == 0) s_base = total[0] ? atomicAdd(flags + CONTACT_COUNT, total[0]) : 0u;
	__syncthreads();
	uint32_t at = s_base + v[0];
#pragma unroll
	for (uint32_t j = 0; j < kContactCompactPer; j++) {
		if (k[j] == kContactEmpty) continue;
		const uint64_t i = i0 + j;
		out_keys[at] = k[j];
#pragma unroll
		for (uint32_t c = 0; c < NC; c++) out_counts[static_cast<uint64_t>(NC) * at + c] = counts[NC * i + c];
		at++;
	}
}

// ------------------------------------------------------------------------------
// overlaps: the contingency table of two streams of one shape, voxels per pair of labels (a of
// the one, b of the other).  No counterpart in the reference.  A pair is constant along the
// intersection of a run of the one stream with a run of the other in the same row of the same
// slice, so no voxel is painted and nothing is sorted: a thread takes one run of stream P, finds
// the run of stream Q that holds its first pixel as contact_row does (Q's word_base and Q's
// vertical-crack plane), walks Q's runs until its last pixel and adds every intersection's
// length to the key (P's label index << 32 | Q's label index).  Each stream is read through its
// own RunGeom / RunArrays: flip, rbase, comp_off and the component counts are the stream's own;
// only sx, sy (hence row_words and plane_words) and the number of slices are shared, which the
// host checks.  The pair table is contacts' scheme with one counter per entry: an LDS table
// per workgroup, flushed into a global one; a key without room in LDS goes to the global table
// directly; a full global table sets a flag and the host doubles it.
// ------------------------------------------------------------------------------
struct OverlapArgs {
	const uint32_t* key_p;           // [total_comp of P] label table index of every component (kNoKey: not in the table)
	const uint32_t* key_q;           // the same of Q
	const uint64_t* comp_off_p;      // [nslices] first component of the slice, per stream
	const uint64_t* comp_off_q;
	const uint32_t* ncomp_p;         // [nslices] components of the slice, per stream
	const uint32_t* ncomp_q;
	uint32_t sx, n_pixels;
	unsigned long long* keys;        // [cap] global table: pair keys, kContactEmpty where free
	unsigned long long* counts;      // [cap] voxels
	uint32_t cap_mask;               // cap - 1, cap a power of two
	uint32_t* flags;                 // [CONTACT_FLAGS], as for contacts
};

// contact_global with one counter
__device__ void overlap_global(const OverlapArgs& oa, unsigned long long key, unsigned long long n) {
	if (__hip_atomic_load(oa.flags + CONTACT_FULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
	const uint32_t h = contact_hash(key);
	for (uint32_t p = 0; p < kContactGlobalProbes && p <= oa.cap_mask; p++) {
		const uint32_t slot = (h + p) & oa.cap_mask;
		unsigned long long cur = oa.keys[slot];      // a slot changes once, from empty to its key: a stale read is settled by the CAS
		if (cur == kContactEmpty) {
			cur = atomicCAS(oa.keys + slot, kContactEmpty, key);
			if (cur == kContactEmpty) cur = key;
		}
		if (cur == key) { atomicAdd(oa.counts + slot, n); return; }
	}
	atomicOr(oa.flags + CONTACT_FULL, 1u);
}

// n voxels with the labels of table indices kp (stream P) and kq (stream Q)
__device__ __forceinline__ void overlap_add(const OverlapArgs& oa, unsigned long long* s_key, uint32_t* s_cnt, uint32_t kp, uint32_t kq, uint32_t n) {
	const unsigned long long key = static_cast<unsigned long long>(kp) << 32 | kq;
	const uint32_t h = contact_hash(key);
	for (uint32_t p = 0; p < kContactProbes; p++) {
		const uint32_t slot = (h + p) & (kContactLds - 1);
		unsigned long long cur = s_key[slot];
		if (cur == kContactEmpty) {
			cur = atomicCAS(s_key + slot, kContactEmpty, key);
			if (cur == kContactEmpty) cur = key;
		}
		if (cur == key) { atomicAdd(s_cnt + slot, n); return; }
	}
	overlap_global(oa, key, n);
}

// grid = (ceil(most runs of a slice of P / kContactRuns), nslices), block = kContactBlock
static __global__ void __launch_bounds__(kContactBlock) k_run_overlaps(RunGeom gq, RunArrays rp, RunArrays rq, OverlapArgs oa) {
	__shared__ unsigned long long s_key[kContactLds];
	// 32 bits are enough: the runs of a workgroup lie in one slice and do not intersect each other,
	// so all that the workgroup adds, to all entries together, is at most the slice's pixels, and
	// those are fewer than 2^32 (n_pixels is a uint32_t).  The global counters are 64 bits wide.
	__shared__ uint32_t s_cnt[kContactLds];
	__shared__ uint32_t s_stop;
	const uint32_t zi = blockIdx.y;
	const uint32_t n = rp.nruns[zi];
	const uint32_t i0 = blockIdx.x * kContactRuns;
	if (i0 >= n) return;
	if (threadIdx.x == 0) s_stop = __hip_atomic_load(oa.flags + CONTACT_FULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	for (uint32_t k = threadIdx.x; k < kContactLds; k += kContactBlock) { s_key[k] = kContactEmpty; s_cnt[k] = 0; }
	__syncthreads();
	if (s_stop) return;      // this pass runs again with a larger table: nothing it adds is kept
	const uint64_t rbp = rp.rbase[zi], rbq = rq.rbase[zi];
	const uint32_t nq = rq.nruns[zi];
	const uint32_t ncp = oa.ncomp_p[zi], ncq = oa.ncomp_q[zi];
	const uint32_t* key_p = oa.key_p + oa.comp_off_p[zi];
	const uint32_t* key_q = oa.key_q + oa.comp_off_q[zi];
	for (uint32_t k = 0; k < kContactPer; k++) {
		const uint32_t i = i0 + k * kContactBlock + threadIdx.x;
		if (i >= n) break;
		const uint32_t a = rp.run_start[rbp + i];
		const uint32_t b = i + 1 < n ? rp.run_start[rbp + i + 1] : oa.n_pixels;
		const uint32_t cc = rp.run_cc[rbp + i];
		const uint32_t kp = cc < ncp ? key_p[cc] : kNoKey;
		// a run outside the slice, or one that is empty or crosses a row's end, would index Q's planes outside them
		if (kp == kNoKey || a >= b || b > oa.n_pixels) { atomicOr(oa.flags + CONTACT_BADKEY, 1u); continue; }
		const uint32_t y = a / oa.sx;
		const uint32_t row = y * oa.sx;
		const uint32_t x0 = a - row, x1 = b - 1 - row;
		if (x1 >= oa.sx) { atomicOr(oa.flags + CONTACT_BADKEY, 1u); continue; }
		const uint32_t w = x0 >> 5;
		uint32_t j = rq.word_base[zi * gq.plane_words + y * gq.row_words + w] + __popc(gq.breaks(zi, y, w) & mask_le(x0 & 31u)) - 1u;
		if (j >= nq) { atomicOr(oa.flags + CONTACT_BADKEY, 1u); continue; }
		uint32_t s = rq.run_start[rbq + j];
		if (s < row || s > a) { atomicOr(oa.flags + CONTACT_BADKEY, 1u); continue; }      // not the run that holds (x0, y)
		s -= row;
		for (;;) {
			// the run after the last one of a row starts the next row (or the slice ends): e <= sx
			const uint32_t e = (j + 1 < nq ? rq.run_start[rbq + j + 1] : oa.n_pixels) - row;
			const uint32_t ccq = rq.run_cc[rbq + j];
			const uint32_t kq = ccq < ncq ? key_q[ccq] : kNoKey;
			const uint32_t hi = min(e, x1 + 1), lo = max(s, x0);
			if (kq == kNoKey || hi <= lo) { atomicOr(oa.flags + CONTACT_BADKEY, 1u); break; }
			overlap_add(oa, s_key, s_cnt, kp, kq, hi - lo);
			if (e > x1) break;
			j++;
			s = e;
		}
	}
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < kContactLds; k += kContactBlock) {
		const unsigned long long key = s_key[k];
		if (key != kContactEmpty) overlap_global(oa, key, s_cnt[k]);
	}
}

#include "ckl_components3d.hpp"

// ------------------------------------------------------------------------------
// voxel connectivity graph (operations.hpp:667-826): bit0 +x, bit1 -x, bit2 +y, bit3 -y from the
// crack planes (a pair across the image border is passable for IMPERMISSIBLE streams and not for
// PERMISSIBLE ones: the reference starts from all-ones / all-zeros and only touches interior
// pairs); connectivity 6 adds bit4 +z / bit5 -z where the decoded labels of neighbouring slices
// agree, and marks the first slice's -z and the last slice's +z.
// grid = (ceil(sxy / 256), nslices); out: x fastest
// ------------------------------------------------------------------------------
template <typename LABEL>
__global__ void __launch_bounds__(kBlock) k_vcg(
	RunGeom g, const LABEL* __restrict__ labels, uint32_t six, uint32_t fortran_order, uint32_t nslices, uint64_t sxy, uint8_t* __restrict__ out
) {
	const uint32_t zi = blockIdx.y;
	const uint64_t p = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
	if (p >= sxy) return;
	const uint32_t y = static_cast<uint32_t>(p / g.sx);
	const uint32_t x = static_cast<uint32_t>(p - static_cast<uint64_t>(y) * g.sx);
	const uint32_t* pv = g.planeV + zi * g.plane_words;
	const uint32_t* ph = g.planeH + zi * g.plane_words;
	// plane bit: crack (IMPERMISSIBLE, flip) or connection (PERMISSIBLE)
	auto joined = [&](const uint32_t* plane, uint32_t px, uint32_t py) -> uint32_t {
		const uint32_t bit = (plane[static_cast<uint64_t>(py) * g.row_words + (px >> 5)] >> (px & 31u)) & 1u;
		return g.flip ? (bit ^ 1u) : bit;
	};
	const uint32_t border = g.flip ? 1u : 0u;
	uint32_t v = 0;
	v |= (x + 1 < g.sx ? joined(pv, x + 1, y) : border) << 0;
	v |= (x >= 1 ? joined(pv, x, y) : border) << 1;
	v |= (y + 1 < g.sy ? joined(ph, x, y + 1) : border) << 2;
	v |= (y >= 1 ? joined(ph, x, y) : border) << 3;
	if (six && nslices > 1) {
		auto at = [&](uint32_t z) -> LABEL {
			return fortran_order ? labels[static_cast<uint64_t>(z) * sxy + p] : labels[z + static_cast<uint64_t>(nslices) * (y + static_cast<uint64_t>(g.sy) * x)];
		};
		const LABEL me = at(zi);
		if (zi + 1 < nslices ? at(zi + 1) == me : true) v |= 0x10u;
		if (zi >= 1 ? at(zi - 1) == me : true) v |= 0x20u;
	}
	out[static_cast<uint64_t>(zi) * sxy + p] = static_cast<uint8_t>(v);
}

// ------------------------------------------------------------------------------
// array_equal (operations.hpp:1039-1184) and mode_pooling_2x2x1 (operations.hpp:1201-1304)
// ------------------------------------------------------------------------------
// one flag: do two device buffers differ anywhere (16 bytes per thread and step, tail by bytes)
__global__ void __launch_bounds__(kBlock) k_buffers_differ(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t n, uint32_t* __restrict__ differ) {
	const uint64_t nv = n / 16;
	uint32_t bad = 0;
	for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < nv; i += static_cast<uint64_t>(gridDim.x) * kBlock) {
		const uint4 x = reinterpret_cast<const uint4*>(a)[i], y = reinterpret_cast<const uint4*>(b)[i];
		bad |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
	}
	if (blockIdx.x == 0 && threadIdx.x < (n & 15u)) bad |= a[nv * 16 + threadIdx.x] ^ b[nv * 16 + threadIdx.x];
	if (bad) atomicOr(differ, 1u);
}

// the reference's 2 x 2 pooling rule (operations.hpp:1254-1290): a == b -> a, a == c -> a, b == c -> b,
// else d; the last column / row of an odd-sized slice is copied.  in: x fastest, one slice after the other
template <typename LABEL>
__global__ void __launch_bounds__(kBlock) k_mode_pool_2x2(const LABEL* __restrict__ in, LABEL* __restrict__ out, uint32_t sx, uint32_t sy, uint32_t nslices) {
	const uint32_t osx = (sx + 1u) >> 1, osy = (sy + 1u) >> 1;
	const uint64_t osxy = static_cast<uint64_t>(osx) * osy, sxy = static_cast<uint64_t>(sx) * sy;
	const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
	if (i >= osxy * nslices) return;
	const uint32_t z = static_cast<uint32_t>(i / osxy);
	const uint32_t r = static_cast<uint32_t>(i - z * osxy);
	const uint32_t oy = r / osx, ox = r - oy * osx;
	const LABEL* src = in + z * sxy;
	const uint32_t x = 2u * ox, y = 2u * oy;
	const bool has_x = x + 1u < sx, has_y = y + 1u < sy;
	const LABEL a = src[x + static_cast<uint64_t>(sx) * y];
	LABEL v = a;
	if (has_x && has_y) {
		const LABEL b = src[x + 1u + static_cast<uint64_t>(sx) * y];
		const LABEL c = src[x + static_cast<uint64_t>(sx) * (y + 1u)];
		const LABEL dd = src[x + 1u + static_cast<uint64_t>(sx) * (y + 1u)];
		v = (a == b) ? a : (a == c) ? a : (b == c) ? b : dd;
	}
	out[i] = v;
}

// ------------------------------------------------------------------------------
// cutout (crackle/array.py:257-285): the labels of an x, y box of every slice of the range.  The
// reference decodes the whole slices and lets numpy crop them; here a paint over the run tables
// writes the box alone, dense, laid out as a decode of a volume that was the box.
// One workgroup per (tile of whole window rows, slice).  The runs a window row crosses are
// consecutive run indices (runs are numbered in raster order): wave 0 finds every row's first and
// last run from word_base and the vertical-crack plane, the labels of those runs (run -> component
// -> label: two dependent loads per run, not per pixel) are staged in LDS row after row, then every
// thread takes chunks of 16 output bytes of consecutive window pixels.  A chunk is aligned to 16
// bytes in the OUTPUT (rows of the box start at any element), so whole chunks are one vector store
// and only the head and the tail of a row go pixel by pixel.  A tile whose rows cross more than
// kWinStage runs (noise) looks every pixel's label up in HBM instead.  Streams that are not
// fortran_order get z fastest, pixel by pixel: correct, not fast.
// Everything read from the tables is clamped: a run to the slice's last one, a component past the
// count of the label section to label 0, as k_paint_runs and k_run_labels do.
// ------------------------------------------------------------------------------
constexpr uint32_t kWinTile = 4096;       // window pixels per workgroup, in whole rows
constexpr uint32_t kWinRows = kWave;      // most rows of a tile: wave 0 holds one row per lane
constexpr uint32_t kWinStage = 1536;      // run labels staged per workgroup

struct WindowArgs {
	uint32_t x0, x1, y0, y1;      // the box in pixels of the slice, x0 < x1 <= sx, y0 < y1 <= sy
	uint32_t rows;                // window rows per tile, 1 .. kWinRows
	uint32_t nslices;
	uint32_t fortran_order;
	uint32_t has_label;           // one byte per voxel: 1 where the label is `label`
	uint64_t label;
};

// grid = (ceil((y1 - y0) / rows), nslices), block = kBlock
template <typename OUT>
__global__ void __launch_bounds__(kBlock) k_paint_window(
	RunGeom g, RunArrays ra, const uint64_t* __restrict__ label_map, const uint64_t* __restrict__ comp_off,
	const uint32_t* __restrict__ ncomp_expect, WindowArgs wa, OUT* __restrict__ out
) {
	constexpr uint32_t V = 16 / sizeof(OUT);      // pixels of a chunk
	struct alignas(16) Chunk { OUT v[V]; };
	__shared__ OUT s_lab[kWinStage];
	__shared__ uint32_t s_lo[kWinRows], s_off[kWinRows + 1];      // per row: its first run, where its labels start in s_lab
	const uint32_t t = threadIdx.x;
	const uint32_t zi = blockIdx.y;
	const uint32_t wx = wa.x1 - wa.x0, wy = wa.y1 - wa.y0;
	const uint32_t r0 = blockIdx.x * wa.rows;
	const uint32_t rows = min(wa.rows, wy - r0);
	const uint32_t nruns = ra.nruns[zi];
	const uint32_t last = nruns ? nruns - 1u : 0u;
	const uint32_t nce = ncomp_expect[zi];
	const uint32_t* rcc = ra.run_cc + ra.rbase[zi];
	const uint64_t* lmap = label_map + comp_off[zi];
	const uint32_t* wb = ra.word_base + zi * g.plane_words;
	auto label_of = [&](uint32_t run) -> OUT {      // run <= last
		if (!nruns) return static_cast<OUT>(0);
		const uint32_t cc = rcc[run];
		uint64_t v = cc < nce ? lmap[cc] : 0ull;
		if (wa.has_label) v = (v == wa.label);
		return static_cast<OUT>(v);
	};
	if (t < kWave) {
		uint32_t lo = 0, n = 0;
		if (t < rows) {
			const uint32_t y = wa.y0 + r0 + t, xe = wa.x1 - 1u;
			lo = min(wb[y * g.row_words + (wa.x0 >> 5)] + __popc(g.breaks(zi, y, wa.x0 >> 5) & mask_le(wa.x0 & 31u)) - 1u, last);
			const uint32_t hi = min(wb[y * g.row_words + (xe >> 5)] + __popc(g.breaks(zi, y, xe >> 5) & mask_le(xe & 31u)) - 1u, last);
			n = hi >= lo ? hi - lo + 1u : 1u;
		}
		uint32_t end = n;      // inclusive scan over the rows
		for (uint32_t d = 1; d < kWave; d <<= 1) {
			const uint32_t o = __shfl_up(end, d, kWave);
			if (t >= d) end += o;
		}
		if (t < rows) { s_lo[t] = lo; s_off[t + 1] = end; }
		if (t == 0) s_off[0] = 0;
	}
	__syncthreads();
	const uint32_t total = s_off[rows];
	const bool staged = total <= kWinStage;
	if (staged) {
		for (uint32_t i = t; i < total; i += kBlock) {
			uint32_t r = 0, hi = rows;      // the row of entry i: the last one that starts at or before it
			while (r + 1 < hi) {
				const uint32_t mid = (r + hi) >> 1;
				if (s_off[mid] <= i) r = mid; else hi = mid;
			}
			s_lab[i] = label_of(min(s_lo[r] + (i - s_off[r]), last));
		}
	}
	__syncthreads();
	// V pixels per 16 bytes of output; a row has a partial chunk in front when it does not start on 16 bytes
	const uint32_t cpr = (wx + V - 1u) / V + 1u;
	const uint32_t nchunks = rows * cpr;
	const uintptr_t base = reinterpret_cast<uintptr_t>(out);
	const bool vec_ok = wa.fortran_order && base % sizeof(OUT) == 0;
	for (uint32_t ci = t; ci < nchunks; ci += kBlock) {
		const uint32_t r = ci / cpr, c = ci - r * cpr;
		const uint32_t wr = r0 + r;
		const uint64_t e0 = (static_cast<uint64_t>(zi) * wy + wr) * wx;      // fortran_order: the row's first element
		const uint32_t mis = vec_ok ? static_cast<uint32_t>((base / sizeof(OUT) + e0) % V) : 0u;
		const uint32_t a = c ? c * V - mis : 0u;
		const uint32_t b = min(wx, (c + 1u) * V - mis);
		if (a >= b) continue;
		const uint32_t n = b - a;
		const uint32_t y = wa.y0 + wr, x = wa.x0 + a, w = x >> 5, sh = x & 31u;
		const uint32_t bw = g.breaks(zi, y, w);
		uint64_t bits = bw >> sh;      // bit j: a run starts at pixel x + j
		if (sh + n > 32u) bits |= static_cast<uint64_t>(g.breaks(zi, y, w + 1u)) << (32u - sh);      // pixel x + n - 1 lies in word w + 1
		uint32_t run = min(wb[y * g.row_words + w] + __popc(bw & mask_le(sh)) - 1u, last);
		Chunk ch;
		if (staged) {
			const uint32_t lo = s_lo[r], k0 = s_off[r], kmax = s_off[r + 1] - 1u;
			uint32_t k = min(k0 + (run >= lo ? run - lo : 0u), kmax);
#pragma unroll
			for (uint32_t j = 0; j < V; j++) {
				if (j) k = min(k + static_cast<uint32_t>((bits >> j) & 1u), kmax);
				ch.v[j] = s_lab[k];
			}
		}
		else {
#pragma unroll
			for (uint32_t j = 0; j < V; j++) {
				if (j) run = min(run + static_cast<uint32_t>((bits >> j) & 1u), last);
				ch.v[j] = j < n ? label_of(run) : static_cast<OUT>(0);
			}
		}
		if (wa.fortran_order) {
			OUT* dst = out + e0 + a;
			if (n == V && vec_ok) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&ch);
			else {
#pragma unroll
				for (uint32_t j = 0; j < V; j++) if (j < n) dst[j] = ch.v[j];
			}
		}
		else {
#pragma unroll
			for (uint32_t j = 0; j < V; j++) if (j < n) out[(static_cast<uint64_t>(a + j) * wy + wr) * wa.nslices + zi] = ch.v[j];
		}
	}
}

}  // namespace ckl

using namespace ckl;

namespace {

// the stream's labels (the unique list of the label section, plus the background colour of a pin
// stream), as the label map holds them (sign-extended), ascending as unsigned: host and device copy
void ensure_label_table(ckl_decoder& d) {
	if (!d.stats_table.empty()) return;
	const Header& h = d.head;
	hipStream_t s = d.stream;
	const int sw = h.stored_data_width;
	std::vector<uint8_t> raw(static_cast<size_t>(d.num_unique) * sw);
	const uint64_t at = h.header_bytes() + h.grid_index_bytes() + d.uniq_offset;
	if (!raw.empty()) CKL_HIP(hipMemcpyAsync(raw.data(), d.d_stream.p + at, raw.size(), hipMemcpyDeviceToHost, s));
	CKL_HIP(hipStreamSynchronize(s));
	std::vector<uint64_t> t(d.num_unique);
	for (uint64_t i = 0; i < d.num_unique; i++) t[i] = read_stored(h, raw.data(), i * sw);
	d.bg_unlisted = h.label_format != FLAT && std::find(t.begin(), t.end(), d.bgcolor) == t.end();
	if (h.label_format != FLAT) t.push_back(d.bgcolor);
	std::sort(t.begin(), t.end());
	t.erase(std::unique(t.begin(), t.end()), t.end());
	d.stats_table.swap(t);
	upload(d.d_stats_table, d.stats_table, s);
	CKL_HIP(hipStreamSynchronize(s));
}

// component -> index into the stream's sorted label table (ensure_label_table), for every component
// of the range after a TABLES run; returns the most runs of one slice
uint32_t component_keys(ckl_decoder& d, DevBuf<uint32_t>& keys) {
	hipStream_t s = d.stream;
	keys.ensure(d.total_comp);
	hipLaunchKernelGGL(k_component_label_index, dim3(static_cast<uint32_t>((d.total_comp + 255) / 256)), dim3(256), 0, s,
		d.d_label_map.p, d.total_comp, d.d_stats_table.p, static_cast<uint32_t>(d.stats_table.size()), keys.p);
	std::vector<uint32_t> nruns(d.nslices);
	CKL_HIP(hipMemcpyAsync(nruns.data(), d.d_nruns.p, d.nslices * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
	CKL_HIP(hipStreamSynchronize(s));
	return *std::max_element(nruns.begin(), nruns.end());
}

// the device span of a whole operation, from the start of its pipeline run, for ckl_decoder_last_timing
void record_span(ckl_decoder& d) {
	CKL_HIP(hipEventRecord(d.ev[kMaxStages + 1], d.stream));
	CKL_HIP(hipEventSynchronize(d.ev[kMaxStages + 1]));
	CKL_HIP(hipEventElapsedTime(&d.pipeline_ms, d.ev[0], d.ev[kMaxStages + 1]));
}

// operations::get_szr (src/operations.hpp:54-72): the clamped z-range of a stream; it must hold a slice
void clamp_range(const Header& h, int64_t z_start, int64_t z_end, int64_t& zs, int64_t& ze) {
	zs = std::max<int64_t>(std::min<int64_t>(z_start, static_cast<int64_t>(static_cast<uint32_t>(h.sz - 1u))), 0);
	ze = z_end < 0 ? static_cast<int64_t>(h.sz) : z_end;
	ze = std::max<int64_t>(std::min<int64_t>(ze, static_cast<int64_t>(h.sz)), 0);
	if (zs >= ze) throw Error(CKL_ERR_RUNTIME, "crackle: Invalid range: " + std::to_string(zs) + " - " + std::to_string(ze));
}

// voxel_counts / centroids / bounding_boxes of the decoded z-range (operations.hpp:321-618):
// one pipeline run up to the run labels, then k_run_stats instead of the paint.
void decoder_label_stats(ckl_decoder& d, uint64_t capacity, uint64_t* labels, uint64_t* counts, uint64_t* sums, uint32_t* boxes, uint64_t* n_out) {
	const Header& h = d.head;
	hipStream_t s = d.stream;
	if (d.sxy == 0 || d.nslices == 0) { *n_out = 0; return; }
	ensure_label_table(d);
	const uint64_t nt = d.stats_table.size();
	*n_out = nt;
	if (capacity < nt) throw Error(CKL_ERR_ARG, "crackle_amd: label statistics need room for " + std::to_string(nt) + " labels");
	d.d_stats_acc.ensure(nt * 4);
	d.d_stats_box.ensure(nt * 6);
	CKL_HIP(hipMemsetAsync(d.d_stats_acc.p, 0, nt * 4 * sizeof(unsigned long long), s));
	hipLaunchKernelGGL(k_stats_init, dim3(static_cast<uint32_t>((nt + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d.d_stats_box.p, static_cast<uint32_t>(nt));
	StatsArgs sa;
	sa.table = d.d_stats_table.p; sa.n_table = static_cast<uint32_t>(nt);
	sa.acc = d.d_stats_acc.p; sa.box = d.d_stats_box.p;
	sa.sx = h.sx; sa.n_pixels = static_cast<uint32_t>(d.sxy); sa.z_start = static_cast<uint32_t>(d.z_start);
	{
		// per-component accumulators in LDS: all of the fullest slice if the workgroup's LDS allows
		uint32_t fit = static_cast<uint32_t>(std::max(0, d.max_lds - 1024)) / kStatsBytesPerComp;
		if (const char* env = getenv("CKL_STATS_LDS_COMPS")) fit = std::min<uint32_t>(fit, static_cast<uint32_t>(std::max(0, atoi(env))));   // testing: forces the run-by-run merge
		sa.lds_comps = std::min<uint32_t>((d.max_comp + 1) & ~1u, fit & ~1u);
		allow_dynamic_lds(reinterpret_cast<const void*>(&k_run_stats), d.device, static_cast<size_t>(sa.lds_comps * kStatsBytesPerComp));
	}
	RunRequest rq = { Goal::STATS };
	rq.stats = &sa;
	decoder_run(d, rq);
	std::vector<unsigned long long> acc(nt * 4);
	CKL_HIP(hipMemcpyAsync(acc.data(), d.d_stats_acc.p, acc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
	if (boxes) CKL_HIP(hipMemcpyAsync(boxes, d.d_stats_box.p, nt * 6 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
	CKL_HIP(hipStreamSynchronize(s));
	for (uint64_t i = 0; i < nt; i++) {
		if (labels) labels[i] = d.stats_table[i];
		if (counts) counts[i] = acc[4 * i];
		if (sums) { sums[3 * i] = acc[4 * i + 1]; sums[3 * i + 1] = acc[4 * i + 2]; sums[3 * i + 2] = acc[4 * i + 3]; }
	}
	// The reference seeds its box map from the unique list only (operations.hpp:561-567); a label outside
	// that list — the background colour of a pin stream — is default-constructed by bbxes[label] when
	// its first component is merged (:596), so its minima start at 0; absent, it has no entry at all
	// (reported here as a zero box with count 0).
	if (boxes && d.bg_unlisted) {
		const uint64_t i = static_cast<uint64_t>(std::lower_bound(d.stats_table.begin(), d.stats_table.end(), d.bgcolor) - d.stats_table.begin());
		if (i < nt && d.stats_table[i] == d.bgcolor) {
			boxes[6 * i] = boxes[6 * i + 1] = boxes[6 * i + 2] = 0;
			if (acc[4 * i] == 0) boxes[6 * i + 3] = boxes[6 * i + 4] = boxes[6 * i + 5] = 0;
		}
	}
}

// voxel_connectivity_graph of the decoder's range into a device buffer of sx*sy*slices bytes
void decoder_vcg(ckl_decoder& d, uint8_t* out_device, uint64_t capacity, int connectivity) {
	const Header& h = d.head;
	if (connectivity != 4 && connectivity != 6) throw Error(CKL_ERR_ARG, "crackle: voxel_connectivity_graph: only connectivity 4 and 6 are currently supported.");
	if (d.sxy == 0 || d.nslices == 0) return;
	const uint64_t need = d.sxy * d.nslices;
	if (!out_device || capacity < need) throw Error(CKL_ERR_ARG, "crackle_amd: output buffer too small: need " + std::to_string(need) + " bytes");
	hipStream_t s = d.stream;
	const bool six = connectivity == 6 && d.nslices > 1;
	DevBuf<uint8_t> labels;
	if (six) {
		// the z bits compare decoded labels: the whole pipeline runs into a scratch volume first
		labels.ensure(need * h.data_width);
		decoder_run(d, { Goal::PAINT, labels.p, need * h.data_width });
	}
	else decoder_run(d, { Goal::PLANES });
	const RunGeom g = run_geom(d);
	const dim3 grid(static_cast<uint32_t>((d.sxy + kBlock - 1) / kBlock), d.nslices);
	const uint32_t f = h.fortran_order ? 1u : 0u;
	with_label_type(h.data_width, [&](auto t) {
		typedef typename decltype(t)::type LABEL;
		hipLaunchKernelGGL(k_vcg<LABEL>, grid, dim3(kBlock), 0, s, g, reinterpret_cast<const LABEL*>(labels.p), six ? 1u : 0u, f, d.nslices, d.sxy, out_device);
	});
	CKL_HIP(hipStreamSynchronize(s));
	CKL_HIP(hipGetLastError());
}

// operations::contacts (src/operations.hpp:850-1021) over the decoder's range: the pairs of touching
// labels (table values, a <= b as unsigned, ascending) and their faces along x, y, z.  One pipeline
// run up to the run tables, then k_run_contacts and k_contacts_compact; a global table that fills
// is cleared and the pass runs again with twice the capacity.
void decoder_contacts(ckl_decoder& d, std::vector<uint64_t>& pairs, std::vector<uint64_t>& faces) {
	const Header& h = d.head;
	hipStream_t s = d.stream;
	const uint32_t ns = d.nslices;
	pairs.clear(); faces.clear();
	if (d.sxy == 0 || ns == 0) return;
	decoder_run(d, { Goal::TABLES });
	ensure_label_table(d);
	const uint32_t n_table = static_cast<uint32_t>(d.stats_table.size());
	if (d.total_comp == 0 || n_table == 0) return;
	DevBuf<uint32_t> d_comp_key;
	const uint32_t max_runs = component_keys(d, d_comp_key);
	if (max_runs == 0) return;

	const RunGeom g = run_geom(d);
	const RunArrays ra = run_arrays(d);

	// First capacity: a label touches some 15 others in a segmentation of compact 3D cells
	// (about 8 pairs per label), twice that as a margin, at most every pair of the table, at a
	// load of 3/4 at most.  Noise, where a label touches most of the others, takes a few doublings.
	const uint64_t est = std::min<uint64_t>(16ull * n_table, static_cast<uint64_t>(n_table) * (n_table + 1) / 2);
	uint64_t cap = 1024;
	while (cap < est + est / 3) cap <<= 1;
	DevBuf<unsigned long long> keys, counts, out_keys, out_counts;
	DevBuf<uint32_t> flags;
	flags.ensure(CONTACT_FLAGS);
	uint32_t hflags[CONTACT_FLAGS];
	for (;;) {
		if (cap > (1ull << 31)) throw Error(CKL_ERR_RUNTIME, "crackle_amd: contacts: more than 2^31 label pairs");
		keys.ensure(cap); counts.ensure(3 * cap); out_keys.ensure(cap); out_counts.ensure(3 * cap);
		CKL_HIP(hipMemsetAsync(keys.p, 0xFF, cap * sizeof(unsigned long long), s));
		CKL_HIP(hipMemsetAsync(counts.p, 0, 3 * cap * sizeof(unsigned long long), s));
		CKL_HIP(hipMemsetAsync(flags.p, 0, CONTACT_FLAGS * sizeof(uint32_t), s));
		ContactArgs ca;
		ca.comp_key = d_comp_key.p;
		ca.zero_key = d.stats_table[0] == 0 ? 0u : kNoKey;
		ca.sx = h.sx; ca.n_pixels = static_cast<uint32_t>(d.sxy);
		ca.keys = keys.p; ca.counts = counts.p;
		ca.cap_mask = static_cast<uint32_t>(cap - 1);
		ca.flags = flags.p;
		hipLaunchKernelGGL(k_run_contacts, dim3((max_runs + kContactRuns - 1) / kContactRuns, ns), dim3(kContactBlock), 0, s,
			g, ra, d.d_comp_off.p, d.d_ncomp_expect.p, ca);
		hipLaunchKernelGGL(k_contacts_compact<3>, dim3(static_cast<uint32_t>((cap + kContactCompact - 1) / kContactCompact)), dim3(kBlock), 0, s,
			keys.p, counts.p, static_cast<uint32_t>(cap), out_keys.p, out_counts.p, flags.p);
		CKL_HIP(hipMemcpyAsync(hflags, flags.p, sizeof(hflags), hipMemcpyDeviceToHost, s));
		CKL_HIP(hipStreamSynchronize(s));
		CKL_HIP(hipGetLastError());
		if (hflags[CONTACT_BADKEY]) throw Error(CKL_ERR_RUNTIME, "crackle_amd: contacts: a component's label is not in the stream's label table");
		if (!hflags[CONTACT_FULL]) break;
		cap <<= 1;
	}
	const uint32_t n = hflags[CONTACT_COUNT];
	std::vector<unsigned long long> k(n), c(3ull * n);
	if (n) {
		CKL_HIP(hipMemcpyAsync(k.data(), out_keys.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
		CKL_HIP(hipMemcpyAsync(c.data(), out_counts.p, 3ull * n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
		CKL_HIP(hipStreamSynchronize(s));
	}
	record_span(d);
	// keys are (index a << 32 | index b) into the ascending table: their order is that of (a, b).
	// Bucketed by a (a label touches a few others), then each bucket sorted by b.
	std::vector<uint32_t> start(n_table + 1, 0), order(n);
	for (uint32_t i = 0; i < n; i++) start[(k[i] >> 32) + 1]++;
	for (uint32_t t = 0; t < n_table; t++) start[t + 1] += start[t];
	{
		std::vector<uint32_t> at(start.begin(), start.end() - 1);
		for (uint32_t i = 0; i < n; i++) order[at[k[i] >> 32]++] = i;
	}
	for (uint32_t t = 0; t < n_table; t++)
		std::sort(order.begin() + start[t], order.begin() + start[t + 1], [&](uint32_t x, uint32_t y) { return k[x] < k[y]; });
	pairs.resize(2ull * n); faces.resize(3ull * n);
	for (uint32_t i = 0; i < n; i++) {
		const unsigned long long key = k[order[i]];
		pairs[2ull * i] = d.stats_table[key >> 32];
		pairs[2ull * i + 1] = d.stats_table[key & 0xFFFFFFFFull];
		for (int a = 0; a < 3; a++) faces[3ull * i + a] = c[3ull * order[i] + a];
	}
}

// First capacity of overlaps' global table for streams of na and nb labels.  Two segmentations of
// compact cells: a cell of the finer one lies inside one cell of the coarser one or straddles a
// face, an edge or a corner between 2, 3 or 4 of them (8 at a lattice corner, rarely), so about 4
// pairs per label of the finer stream are a generous mean; every label of the coarser one has a
// pair as well.  At most every pair of the two tables, at a load of 3/4 at most.  Noise against
// noise, where nearly every voxel is a pair of its own, takes a few doublings.
uint64_t overlap_first_capacity(uint64_t na, uint64_t nb) {
	const uint64_t est = std::min<uint64_t>(4 * std::max(na, nb) + std::min(na, nb), na * nb);
	uint64_t cap = 1024;
	while (cap < est + est / 3) cap <<= 1;
	return cap;
}

// The contingency table of two sessions of one slice shape and one number of slices, slice i of the
// one against slice i of the other: pairs (a, b) of label values, ascending as unsigned, and their
// voxels.  A TABLES run of each, then k_run_overlaps over the runs of the stream whose fullest slice
// has more of them (the walk along the other stream's runs is then the short one; the key halves are
// swapped back here) and k_contacts_compact; a global table that fills runs the pass again, doubled.
struct OverlapTable {
	HostOut<uint64_t> pairs, counts;      // 2 n and n values; unset while n is 0
	uint64_t n = 0;
};
void decoder_overlaps(ckl_decoder& a, ckl_decoder& b, OverlapTable& out) {
	if (a.device != b.device) throw Error(CKL_ERR_ARG, "crackle_amd: overlaps: the sessions are on different devices: " + std::to_string(a.device) + " and " + std::to_string(b.device));
	if (a.head.sx != b.head.sx || a.head.sy != b.head.sy || a.nslices != b.nslices)
		throw Error(CKL_ERR_ARG, "crackle_amd: overlaps: the sessions differ in shape: " + std::to_string(a.head.sx) + " x " + std::to_string(a.head.sy) + " x " + std::to_string(a.nslices)
			+ " slices and " + std::to_string(b.head.sx) + " x " + std::to_string(b.head.sy) + " x " + std::to_string(b.nslices) + " slices");
	if (a.sxy == 0 || a.nslices == 0) return;
	// a's pipeline starts the span that record_span closes; every step on b's stream is waited for by
	// the host (component_keys at the latest) before the kernels that read b's tables go to a's stream
	decoder_run(a, { Goal::TABLES });
	if (&b != &a) decoder_run(b, { Goal::TABLES });
	ensure_label_table(a);
	ensure_label_table(b);
	const uint32_t na = static_cast<uint32_t>(a.stats_table.size()), nb = static_cast<uint32_t>(b.stats_table.size());
	if (a.total_comp == 0 || b.total_comp == 0 || na == 0 || nb == 0) return;
	DevBuf<uint32_t> d_key_a, d_key_b;
	const uint32_t max_a = component_keys(a, d_key_a), max_b = component_keys(b, d_key_b);
	if (max_a == 0 || max_b == 0) return;
	const bool swapped = max_b > max_a;
	ckl_decoder& p = swapped ? b : a;
	ckl_decoder& q = swapped ? a : b;
	const RunGeom gp = run_geom(p), gq = run_geom(q);
	if (gp.row_words != gq.row_words || gp.plane_words != gq.plane_words || gp.sx != gq.sx || gp.sy != gq.sy || p.sxy != q.sxy)
		throw Error(CKL_ERR_RUNTIME, "crackle_amd: overlaps: the sessions' crack planes differ in layout");
	const RunArrays rp = run_arrays(p), rq = run_arrays(q);
	hipStream_t s = a.stream;

	uint64_t cap = overlap_first_capacity(na, nb);
	DevBuf<unsigned long long> keys, cnt, out_keys, out_cnt;
	DevBuf<uint32_t> flags;
	flags.ensure(CONTACT_FLAGS);
	uint32_t hflags[CONTACT_FLAGS];
	for (;;) {
		if (cap > (1ull << 31)) throw Error(CKL_ERR_RUNTIME, "crackle_amd: overlaps: more than 2^31 label pairs");
		keys.ensure(cap); cnt.ensure(cap); out_keys.ensure(cap); out_cnt.ensure(cap);
		CKL_HIP(hipMemsetAsync(keys.p, 0xFF, cap * sizeof(unsigned long long), s));
		CKL_HIP(hipMemsetAsync(cnt.p, 0, cap * sizeof(unsigned long long), s));
		CKL_HIP(hipMemsetAsync(flags.p, 0, CONTACT_FLAGS * sizeof(uint32_t), s));
		OverlapArgs oa;
		oa.key_p = swapped ? d_key_b.p : d_key_a.p; oa.key_q = swapped ? d_key_a.p : d_key_b.p;
		oa.comp_off_p = p.d_comp_off.p; oa.comp_off_q = q.d_comp_off.p;
		oa.ncomp_p = p.d_ncomp_expect.p; oa.ncomp_q = q.d_ncomp_expect.p;
		oa.sx = p.head.sx; oa.n_pixels = static_cast<uint32_t>(p.sxy);
		oa.keys = keys.p; oa.counts = cnt.p;
		oa.cap_mask = static_cast<uint32_t>(cap - 1);
		oa.flags = flags.p;
		hipLaunchKernelGGL(k_run_overlaps, dim3((std::max(max_a, max_b) + kContactRuns - 1) / kContactRuns, p.nslices), dim3(kContactBlock), 0, s, gq, rp, rq, oa);
		hipLaunchKernelGGL(k_contacts_compact<1>, dim3(static_cast<uint32_t>((cap + kContactCompact - 1) / kContactCompact)), dim3(kBlock), 0, s,
			keys.p, cnt.p, static_cast<uint32_t>(cap), out_keys.p, out_cnt.p, flags.p);
		CKL_HIP(hipMemcpyAsync(hflags, flags.p, sizeof(hflags), hipMemcpyDeviceToHost, s));
		CKL_HIP(hipStreamSynchronize(s));
		CKL_HIP(hipGetLastError());
		if (hflags[CONTACT_BADKEY]) throw Error(CKL_ERR_RUNTIME, "crackle_amd: overlaps: a run or a component's label is outside the stream's tables");
		if (!hflags[CONTACT_FULL]) break;
		cap <<= 1;
	}
	const uint32_t n = hflags[CONTACT_COUNT];
	auto k = host_out<unsigned long long>(std::max<uint32_t>(n, 1)), c = host_out<unsigned long long>(std::max<uint32_t>(n, 1));
	if (n) {
		CKL_HIP(hipMemcpyAsync(k.get(), out_keys.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
		CKL_HIP(hipMemcpyAsync(c.get(), out_cnt.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
		CKL_HIP(hipStreamSynchronize(s));
	}
	record_span(a);
	// Indices into ascending label tables: the order of (index a, index b) is that of the label pairs.
	// The entries are moved into buckets by a (one counting pass), then each bucket, a few entries that
	// lie together, is sorted by b.
	struct Entry { uint32_t kb; unsigned long long n; };
	const uint32_t sh_a = swapped ? 0 : 32, sh_b = swapped ? 32 : 0;
	std::vector<uint32_t> start(na + 1, 0);
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t ka = static_cast<uint32_t>(k[i] >> sh_a), kb = static_cast<uint32_t>(k[i] >> sh_b);
		if (ka >= na || kb >= nb) throw Error(CKL_ERR_RUNTIME, "crackle_amd: overlaps: a pair outside the streams' label tables");
		start[ka + 1]++;
	}
	for (uint32_t t = 0; t < na; t++) start[t + 1] += start[t];
	auto entry = host_out<Entry>(std::max<uint32_t>(n, 1));      // (a cached block of the host pool)
	{
		std::vector<uint32_t> at(start.begin(), start.end() - 1);
		for (uint32_t i = 0; i < n; i++) entry[at[static_cast<uint32_t>(k[i] >> sh_a)]++] = { static_cast<uint32_t>(k[i] >> sh_b), c[i] };
	}
	out.pairs = host_out<uint64_t>(std::max<uint64_t>(2ull * n, 1));
	out.counts = host_out<uint64_t>(std::max<uint32_t>(n, 1));
	out.n = n;
	for (uint32_t t = 0; t < na; t++) {
		if (start[t + 1] - start[t] > 1) std::sort(entry.get() + start[t], entry.get() + start[t + 1], [](const Entry& x, const Entry& y) { return x.kb < y.kb; });
		const uint64_t va = a.stats_table[t];
		for (uint32_t i = start[t]; i < start[t + 1]; i++) {
			out.pairs[2ull * i] = va;
			out.pairs[2ull * i + 1] = b.stats_table[entry[i].kb];
			out.counts[i] = entry[i].n;
		}
	}
}

// connected_components over the whole stream (ckl_components3d.hpp): one pipeline run up to the run
// tables and the component -> label map, the links, the numbering.  keys: one key per component at
// key_width bytes into the list 0, 1 .. n_components (has_zero) or 1 .. n_components;
// root_labels (when wanted): the original label of every numbered component.
struct Components3D {
	std::vector<uint8_t> keys;
	int key_width = 1;
	uint64_t n_components = 0;
	bool has_zero = false;
	std::vector<uint64_t> root_labels;
};

// The front that connected_components and dust share: one pipeline run up to the run tables, the
// label table, every component's label index, the links, the roots.  flags is cleared before the
// links and holds CC_BADKEY after them (read together with what the caller's kernels add).
struct ComponentLinks {
	DevBuf<uint32_t> comp_key, parent, root, flags;
	uint32_t nc = 0, zero_key = kNoKey, max_runs = 0;
};

// mode: what k_run_links unites (LINK_BY_LABEL, LINK_FOREGROUND for dust's binary_image, LINK_BACKGROUND for fill_holes)
void link_components(ckl_decoder& d, int connectivity, uint32_t mode, const char* what, ComponentLinks& L) {
	const Header& h = d.head;
	hipStream_t s = d.stream;
	decoder_run(d, { Goal::TABLES });
	ensure_label_table(d);
	const uint32_t n_table = static_cast<uint32_t>(d.stats_table.size());
	if (d.total_comp == 0 || n_table == 0) throw Error(CKL_ERR_RUNTIME, "crackle: label section is malformed or corrupted.");
	if (d.total_comp > 0xFFFFFFFFull) throw Error(CKL_ERR_RUNTIME, std::string("crackle_amd: ") + what + ": more than 2^32 - 1 components");
	const uint32_t nc = L.nc = static_cast<uint32_t>(d.total_comp);
	L.max_runs = component_keys(d, L.comp_key);
	const RunGeom g = run_geom(d);
	const RunArrays ra = run_arrays(d);
	L.parent.ensure(nc); L.root.ensure(nc); L.flags.ensure(CC_FLAGS);
	CKL_HIP(hipMemsetAsync(L.flags.p, 0, CC_FLAGS * sizeof(uint32_t), s));
	LinkArgs la;
	la.comp_key = L.comp_key.p;
	la.zero_key = L.zero_key = d.stats_table[0] == 0 ? 0u : kNoKey;
	la.sx = h.sx; la.sy = h.sy; la.n_pixels = static_cast<uint32_t>(d.sxy);
	la.connectivity = static_cast<uint32_t>(connectivity);
	la.mode = mode;
	la.parent = L.parent.p; la.flags = L.flags.p;
	hipLaunchKernelGGL(k_cc_init, dim3((nc + kBlock - 1) / kBlock), dim3(kBlock), 0, s, L.parent.p, nc);
	if (L.max_runs) hipLaunchKernelGGL(k_run_links, dim3((L.max_runs + kContactRuns - 1) / kContactRuns, d.nslices), dim3(kContactBlock), 0, s,
		g, ra, d.d_comp_off.p, d.d_ncomp_expect.p, la);
	hipLaunchKernelGGL(k_cc_flatten, dim3((nc + kBlock - 1) / kBlock), dim3(kBlock), 0, s, L.parent.p, nc, L.root.p);
}

void decoder_connected_components(ckl_decoder& d, int connectivity, bool want_labels, Components3D& out) {
	hipStream_t s = d.stream;
	ComponentLinks L;
	link_components(d, connectivity, LINK_BY_LABEL, "connected_components", L);
	const uint32_t nc = L.nc;
	DevBuf<uint32_t> number, blk;
	DevBuf<uint64_t> root_label;
	DevBuf<uint8_t> keys;
	const uint32_t nb = (nc + kCcTile - 1) / kCcTile;
	number.ensure(nc); blk.ensure(nb);
	if (want_labels) root_label.ensure(nc);
	keys.ensure(4ull * nb * kCcTile);      // the widest keys, padded to whole tiles
	hipLaunchKernelGGL(k_cc_count, dim3(nb), dim3(kBlock), 0, s, L.root.p, L.comp_key.p, L.zero_key, nc, blk.p, L.flags.p);
	hipLaunchKernelGGL(k_cc_offsets, dim3(1), dim3(kBlock), 0, s, blk.p, nb, L.flags.p);
	hipLaunchKernelGGL(k_cc_number, dim3(nb), dim3(kBlock), 0, s, L.root.p, L.comp_key.p, L.zero_key, nc, blk.p, number.p,
		d.d_label_map.p, want_labels ? reinterpret_cast<uint64_t*>(root_label.p) : nullptr);
	hipLaunchKernelGGL(k_cc_keys, dim3(nb), dim3(kBlock), 0, s, L.root.p, L.comp_key.p, L.zero_key, nc, number.p, L.flags.p, keys.p);
	uint32_t hflags[CC_FLAGS];
	CKL_HIP(hipMemcpyAsync(hflags, L.flags.p, sizeof(hflags), hipMemcpyDeviceToHost, s));
	CKL_HIP(hipStreamSynchronize(s));
	CKL_HIP(hipGetLastError());
	if (hflags[CC_BADKEY]) throw Error(CKL_ERR_RUNTIME, "crackle_amd: connected_components: a component's label is not in the stream's label table");
	out.n_components = hflags[CC_COUNT];
	out.has_zero = hflags[CC_HAS_ZERO] != 0;
	out.key_width = byte_width(out.n_components + (out.has_zero ? 1 : 0));
	out.keys.resize(static_cast<size_t>(nc) * out.key_width);
	CKL_HIP(hipMemcpyAsync(out.keys.data(), keys.p, out.keys.size(), hipMemcpyDeviceToHost, s));
	out.root_labels.resize(want_labels ? out.n_components : 0);
	if (want_labels && out.n_components) CKL_HIP(hipMemcpyAsync(out.root_labels.data(), root_label.p, out.n_components * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
	record_span(d);
}

// The label edit that dust and fill_holes end with (k_edit_mark / k_edit_keys of ckl_components3d.hpp): every
// component's new label is decided on the device by `edit`; the new unique list is made on the host from one
// byte per label of the old one, the device packs the keys.  uniq: the new list, ascending; keys: one key per
// component at key_width bytes; n_changed: the 3D components whose label changed.
struct LabelEdit {
	std::vector<uint64_t> uniq;
	std::vector<uint8_t> keys;
	int key_width = 1;
	uint64_t n_changed = 0;
};

// (flags: CC_BADKEY of the kernels before is read here; CC_COUNT must be 0 on entry)
template <typename Edit>
static void edit_labels(ckl_decoder& d, ComponentLinks& L, const Edit& edit, const char* what, LabelEdit& out) {
	hipStream_t s = d.stream;
	const uint32_t nc = L.nc;
	const uint32_t n_table = static_cast<uint32_t>(d.stats_table.size());
	DevBuf<uint8_t> used, keys;
	DevBuf<uint32_t> new_index;
	used.ensure(n_table);
	CKL_HIP(hipMemsetAsync(used.p, 0, n_table, s));
	hipLaunchKernelGGL(k_edit_mark<Edit>, dim3((nc + kBlock - 1) / kBlock), dim3(kBlock), 0, s, edit, n_table, used.p, L.flags.p);
	uint32_t hflags[CC_FLAGS];
	std::vector<uint8_t> hused(n_table);
	CKL_HIP(hipMemcpyAsync(hflags, L.flags.p, sizeof(hflags), hipMemcpyDeviceToHost, s));
	CKL_HIP(hipMemcpyAsync(hused.data(), used.p, n_table, hipMemcpyDeviceToHost, s));
	CKL_HIP(hipStreamSynchronize(s));
	CKL_HIP(hipGetLastError());
	if (hflags[CC_BADKEY]) throw Error(CKL_ERR_RUNTIME, std::string("crackle_amd: ") + what + ": a component's label is not in the stream's label table");
	out.n_changed = hflags[CC_COUNT];
	// the labels still in use, ascending as the table is; 0 in front when a component got it and it was not there
	const bool add_zero = Edit::kGivesZero && out.n_changed != 0 && !(L.zero_key != kNoKey && hused[L.zero_key]);
	std::vector<uint32_t> index(n_table, 0);
	out.uniq.clear();
	if (add_zero) out.uniq.push_back(0);
	for (uint32_t k = 0; k < n_table; k++) {
		if (!hused[k]) continue;
		index[k] = static_cast<uint32_t>(out.uniq.size());
		out.uniq.push_back(d.stats_table[k]);
	}
	if (out.uniq.empty() || out.uniq.size() > 0xFFFFFFFFull) throw Error(CKL_ERR_RUNTIME, std::string("crackle_amd: ") + what + ": the new label list is empty or holds 2^32 labels or more");
	out.key_width = byte_width(out.uniq.size());
	upload(new_index, index, s);
	const uint32_t nq = (nc + 3) / 4;      // four components per thread
	keys.ensure(16ull * nq);              // the widest keys, padded to a multiple of four
	hipLaunchKernelGGL(k_edit_keys<Edit>, dim3((nq + kBlock - 1) / kBlock), dim3(kBlock), 0, s, edit, n_table, new_index.p, static_cast<uint32_t>(out.uniq.size()), keys.p);
	out.keys.resize(static_cast<size_t>(nc) * out.key_width);
	CKL_HIP(hipMemcpyAsync(out.keys.data(), keys.p, out.keys.size(), hipMemcpyDeviceToHost, s));
	CKL_HIP(hipStreamSynchronize(s));
	CKL_HIP(hipGetLastError());
	record_span(d);
}

// dust over the whole stream (ckl_components3d.hpp): the links of connected_components (by label, or
// binary_image: between any two foreground voxels), the voxels of every set (k_cc_voxels), then the
// label edit: a component of a set below the threshold (invert: at or above it) gets label 0.
void decoder_dust(ckl_decoder& d, uint64_t threshold, int connectivity, bool binary_image, bool invert, LabelEdit& out) {
	hipStream_t s = d.stream;
	ComponentLinks L;
	link_components(d, connectivity, binary_image ? LINK_FOREGROUND : LINK_BY_LABEL, "dust", L);
	const uint32_t nc = L.nc;
	DevBuf<unsigned long long> voxels;
	voxels.ensure(nc);
	CKL_HIP(hipMemsetAsync(voxels.p, 0, nc * sizeof(unsigned long long), s));
	VoxelArgs va;
	va.comp_key = L.comp_key.p; va.zero_key = L.zero_key;
	va.n_pixels = static_cast<uint32_t>(d.sxy);
	va.root = L.root.p; va.voxels = voxels.p; va.flags = L.flags.p;
	if (L.max_runs) hipLaunchKernelGGL(k_cc_voxels, dim3((L.max_runs + kContactRuns - 1) / kContactRuns, d.nslices), dim3(kContactBlock), 0, s,
		run_arrays(d), d.d_comp_off.p, d.d_ncomp_expect.p, va);
	DustArgs da;
	da.root = L.root.p; da.comp_key = L.comp_key.p; da.voxels = voxels.p;
	da.zero_key = L.zero_key; da.n = nc;
	da.threshold = threshold; da.invert = invert ? 1u : 0u;
	edit_labels(d, L, da, "dust", out);
}

// fill_holes over the whole stream (ckl_components3d.hpp): the links of label 0's components at the wanted
// connectivity, one state word per background set from the face neighbours of its runs (k_hole_scan), then the
// label edit: a component of a set that lies on no face of the volume and saw exactly one label gets that label.
void decoder_fill_holes(ckl_decoder& d, int connectivity, LabelEdit& out) {
	hipStream_t s = d.stream;
	const Header& h = d.head;
	ComponentLinks L;
	link_components(d, connectivity, LINK_BACKGROUND, "fill_holes", L);
	if (d.nslices != h.sz) throw Error(CKL_ERR_RUNTIME, "crackle_amd: fill_holes: the decoder does not cover the whole volume");
	if (d.stats_table.size() >= HOLE_MANY - 1u) throw Error(CKL_ERR_RUNTIME, "crackle_amd: fill_holes: 2^32 - 3 labels or more");
	const uint32_t nc = L.nc;
	DevBuf<uint32_t> state;
	state.ensure(nc);
	CKL_HIP(hipMemsetAsync(state.p, 0, nc * sizeof(uint32_t), s));
	if (L.max_runs && L.zero_key != kNoKey) {
		HoleArgs ha;
		ha.comp_key = L.comp_key.p; ha.zero_key = L.zero_key;
		ha.sx = h.sx; ha.sy = h.sy; ha.n_pixels = static_cast<uint32_t>(d.sxy); ha.nslices = d.nslices;
		ha.root = L.root.p; ha.state = state.p; ha.flags = L.flags.p;
		hipLaunchKernelGGL(k_hole_scan, dim3((L.max_runs + kContactRuns - 1) / kContactRuns, d.nslices), dim3(kContactBlock), 0, s,
			run_geom(d), run_arrays(d), d.d_comp_off.p, d.d_ncomp_expect.p, ha);
	}
	FillArgs fa;
	fa.root = L.root.p; fa.comp_key = L.comp_key.p; fa.state = state.p;
	fa.zero_key = L.zero_key; fa.n = nc;
	edit_labels(d, L, fa, "fill_holes", out);
}

// operations::point_cloud (src/operations.hpp:183-262): contours of every component of the decoder's
// range (ckl_contours.hpp), grouped by label.  The pipeline runs up to the run tables and the
// component -> label map (the integrity check's mode), then per z-chunk: direction masks, the
// per-slice tracer, the contours' components; the host orders the contours of each component
// (dual_graph.hpp:223-241), groups components by label in (z, component) order and plans the
// output, which k_contour_emit writes on the device.
struct PointCloud {
	std::vector<uint64_t> labels;      // ascending
	std::vector<uint64_t> offsets;     // [labels + 1], in points
	HostOut<uint16_t> points;          // 3 uint16 per point
};

void decoder_point_cloud(ckl_decoder& d, const uint64_t* sel, uint64_t n_sel, bool has_sel, bool skip_background, PointCloud& out) {
	const Header& h = d.head;
	hipStream_t s = d.stream;
	const uint32_t ns = d.nslices;
	out.offsets.assign(1, 0);
	if (d.sxy == 0 || ns == 0) return;
	// The most contour nodes the tracer keeps for one slice.  A walk is one orbit of the wall
	// follower on the darts (directed edges) of the 4-connected pixel graph: it never passes a dart
	// twice and stores one node per step plus its start.  The walks in either sense of one loop
	// pass the same pixels, so a loop is kept at most once (dual_graph.hpp:199-201), and every dart
	// lies on one loop: the kept walks store at most 2 E nodes, E = 2 sx sy - sx - sy edges, plus
	// one start per kept contour, at most one per pixel (each passes a pixel not passed before).
	// Dropped walks store nothing past the buffer (k_trace_contours).  raw and the kernel's tail
	// and room are 32-bit: larger slices are refused.
	const uint64_t raw_worst = 2 * (2 * d.sxy - h.sx - h.sy) + d.sxy;
	if (raw_worst > 0xFFFFFFFFull) throw Error(CKL_ERR_ARG, "crackle_amd: point_cloud: slices of 2^32 contour nodes or more (5 sx sy - 2 sx - 2 sy) are not supported");
	decoder_run(d, { Goal::TABLES });
	const RunGeom g = run_geom(d);
	const RunArrays ra = run_arrays(d);

	// component -> label as an index into the stream's sorted label table (binary search on the
	// device); point_cloud<LABEL> keys its map by the unsigned type of the data width, which keeps
	// the table's order (sign-extended labels, ascending as unsigned)
	ensure_label_table(d);
	const uint32_t n_table = static_cast<uint32_t>(d.stats_table.size());
	std::vector<uint32_t> comp_key(d.total_comp);
	if (d.total_comp) {
		DevBuf<uint32_t> d_comp_key;
		component_keys(d, d_comp_key);
		CKL_HIP(hipMemcpyAsync(comp_key.data(), d_comp_key.p, d.total_comp * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
		CKL_HIP(hipStreamSynchronize(s));
	}
	const uint64_t lmask = h.data_width >= 8 ? ~0ull : ((1ull << (8 * h.data_width)) - 1);
	std::vector<uint64_t> comp_off(ns + 1, 0);
	for (uint32_t zi = 0; zi < ns; zi++) comp_off[zi + 1] = comp_off[zi] + d.ncomp_expect_host[zi];
	std::vector<uint64_t> selected;
	if (has_sel) { selected.assign(sel, sel + n_sel); std::sort(selected.begin(), selected.end()); }
	auto takes = [&](uint64_t label) {
		if (skip_background && label == 0) return false;
		return !has_sel || std::binary_search(selected.begin(), selected.end(), label);
	};

	const bool prof = getenv("CKL_PROFILE") != nullptr;
	auto t_last = std::chrono::steady_clock::now();
	std::string marks;
	auto mark = [&](const char* name) {
		if (!prof) return;
		CKL_HIP(hipStreamSynchronize(s));
		const auto now = std::chrono::steady_clock::now();
		char buf[64];
		snprintf(buf, sizeof buf, " %s=%.2f", name, std::chrono::duration<double, std::milli>(now - t_last).count());
		marks += buf;
		t_last = now;
	};
	mark("tables");
	uint64_t walk_steps = 0;
	const uint32_t sxy = static_cast<uint32_t>(d.sxy);
	const uint64_t dirs_stride = (d.sxy + 3) & ~3ull;
	const uint32_t vis_words = (sxy + 31) / 32;
	const uint32_t cand_words = ((vis_words + 1) & ~1u) + 2 * kContourWindow;      // a scan window may start at the last word
	const bool lds_vis = !getenv("CKL_CONTOUR_HBM_VISITED") && static_cast<uint64_t>(vis_words) * 4 + 256 <= static_cast<uint64_t>(std::max(0, d.max_lds));
	if (lds_vis) allow_dynamic_lds(reinterpret_cast<const void*>(&k_trace_contours<true>), d.device, static_cast<size_t>(vis_words * 4));

	// contours of all slices: per slice the kept ones in discovery order
	struct Kept { uint32_t zi, offset, len, rot, first, comp; };
	std::vector<Kept> kept;
	// per z-chunk device buffers, kept until the emit; first try with room for the usual volume,
	// a chunk that overflows is traced again with the bounds of the worst case
	struct Chunk { uint32_t z0, n; uint32_t raw_cap; std::unique_ptr<DevBuf<uint32_t>> raw; };
	std::vector<Chunk> chunks;
	const uint64_t budget = 3ull << 30;
	uint32_t raw_cap0 = static_cast<uint32_t>(std::min<uint64_t>(d.sxy / 2 + 4096, raw_worst));
	uint32_t tab_cap0 = static_cast<uint32_t>(std::min<uint64_t>(d.sxy / 32 + 1024, d.sxy + 1));
	if (const char* env = getenv("CKL_CONTOUR_SMALL")) { raw_cap0 = std::max(16, atoi(env)); tab_cap0 = std::max(2, atoi(env) / 8); }      // testing: forces the second pass
	DevBuf<uint8_t> d_dirs;
	DevBuf<uint32_t> d_vis, d_counts, d_comp, d_cand, d_walked;
	DevBuf<uint4> d_table;
	uint32_t z0 = 0;
	while (z0 < ns) {
		uint32_t raw_cap = raw_cap0, tab_cap = tab_cap0;
		for (int attempt = 0; ; attempt++) {
			const uint64_t per_slice = dirs_stride + 4ull * vis_words + 8ull * cand_words + 4ull * raw_cap + 16ull * tab_cap + 4ull * tab_cap + (lds_vis ? 0 : 4ull * vis_words) + 16;
			const uint32_t nz = static_cast<uint32_t>(std::min<uint64_t>(ns - z0, std::max<uint64_t>(1, budget / per_slice)));
			RunGeom gz = g;
			gz.planeV = g.planeV + static_cast<uint64_t>(z0) * d.plane_words;
			gz.planeH = g.planeH + static_cast<uint64_t>(z0) * d.plane_words;
			RunArrays rz = ra;
			rz.word_base = ra.word_base + static_cast<uint64_t>(z0) * d.plane_words;
			rz.rbase = ra.rbase + z0;
			d_dirs.ensure(dirs_stride * nz);
			std::unique_ptr<DevBuf<uint32_t>> raw(new DevBuf<uint32_t>());
			raw->ensure(static_cast<uint64_t>(raw_cap) * nz);
			d_table.ensure(static_cast<uint64_t>(tab_cap) * nz);
			d_comp.ensure(static_cast<uint64_t>(tab_cap) * nz);
			d_counts.ensure(4ull * nz);
			if (!lds_vis) {
				d_vis.ensure(static_cast<uint64_t>(vis_words) * nz);
				CKL_HIP(hipMemsetAsync(d_vis.p, 0, static_cast<uint64_t>(vis_words) * nz * sizeof(uint32_t), s));
			}
			d_cand.ensure(2ull * cand_words * nz);
			CKL_HIP(hipMemsetAsync(d_cand.p, 0, 2ull * cand_words * nz * sizeof(uint32_t), s));
			hipLaunchKernelGGL(k_contour_dirs, dim3(static_cast<uint32_t>((d.sxy + 255) / 256), nz), dim3(256), 0, s, gz, d.sxy, dirs_stride, d_dirs.p,
				cand_words, d_cand.p, d_cand.p + static_cast<uint64_t>(cand_words) * nz);
			mark("dirs");
			const bool memo = !getenv("CKL_CONTOUR_NO_MEMO");      // testing: every start is walked, like the reference does
			if (memo) {
				d_walked.ensure(static_cast<uint64_t>(vis_words) * nz);
				CKL_HIP(hipMemsetAsync(d_walked.p, 0, static_cast<uint64_t>(vis_words) * nz * sizeof(uint32_t), s));
			}
			ContourArgs ca;
			ca.walked_r = memo ? d_walked.p : nullptr;
			ca.cand_a = d_cand.p; ca.cand_b = d_cand.p + static_cast<uint64_t>(cand_words) * nz; ca.cand_words = cand_words;
			ca.dirs = d_dirs.p; ca.visited = d_vis.p; ca.raw = raw->p; ca.table = d_table.p; ca.counts = d_counts.p;
			ca.sx = h.sx; ca.sy = h.sy; ca.sxy = sxy; ca.raw_cap = raw_cap; ca.tab_cap = tab_cap; ca.vis_words = vis_words; ca.dirs_stride = dirs_stride;
			if (lds_vis) hipLaunchKernelGGL(k_trace_contours<true>, dim3(nz), dim3(64), vis_words * 4, s, ca);
			else hipLaunchKernelGGL(k_trace_contours<false>, dim3(nz), dim3(64), 0, s, ca);
			mark("trace");
			hipLaunchKernelGGL(k_contour_components, dim3((tab_cap + 255) / 256, nz), dim3(256), 0, s, gz, rz, d_table.p, d_counts.p, tab_cap, d_comp.p);
			std::vector<uint32_t> counts(4ull * nz);
			CKL_HIP(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
			CKL_HIP(hipStreamSynchronize(s));
			CKL_HIP(hipGetLastError());
			uint32_t flags = 0;
			for (uint32_t i = 0; i < nz; i++) { flags |= counts[4 * i + 2]; walk_steps += counts[4 * i + 3]; }
			if (flags & kContourOpenWalk) throw Error(CKL_ERR_RUNTIME, "crackle_amd: point_cloud: a contour walk did not close");
			if (flags) {
				if (attempt) throw Error(CKL_ERR_RUNTIME, "crackle_amd: point_cloud: contour buffers overflow");
				raw_cap = static_cast<uint32_t>(std::max<uint64_t>(raw_worst, 1));
				tab_cap = sxy + 1;
				continue;
			}
			// the kept contours of the chunk, packed on the device: one copy instead of one per slice
			std::vector<uint32_t> base(nz + 1, 0);
			for (uint32_t i = 0; i < nz; i++) base[i + 1] = base[i] + counts[4 * i];
			const uint32_t n_chunk = base[nz];
			if (n_chunk) {
				DevBuf<uint32_t> d_base, d_pcomp;
				DevBuf<uint4> d_ptable;
				upload(d_base, base, s);
				d_ptable.ensure(n_chunk); d_pcomp.ensure(n_chunk);
				hipLaunchKernelGGL(k_contour_pack, dim3((tab_cap + 255) / 256, nz), dim3(256), 0, s, d_table.p, d_comp.p, d_counts.p, d_base.p, tab_cap, d_ptable.p, d_pcomp.p);
				std::vector<uint4> table(n_chunk);
				std::vector<uint32_t> comp(n_chunk);
				CKL_HIP(hipMemcpyAsync(table.data(), d_ptable.p, n_chunk * sizeof(uint4), hipMemcpyDeviceToHost, s));
				CKL_HIP(hipMemcpyAsync(comp.data(), d_pcomp.p, n_chunk * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
				CKL_HIP(hipStreamSynchronize(s));
				const size_t at0 = kept.size();
				kept.resize(at0 + n_chunk);
				for (uint32_t i = 0; i < nz; i++) {
					for (uint32_t k = base[i]; k < base[i + 1]; k++) {
						const uint4 t = table[k];
						kept[at0 + k] = { z0 + i, t.x, t.y, t.z, t.w, comp[k] };
					}
				}
			}
			chunks.push_back({ z0, nz, raw_cap, std::move(raw) });
			z0 += nz;
			break;
		}
	}

	mark("collect");
	// merge_contours_via_vcg_coloring (dual_graph.hpp:213-243): a contour whose first node lies before
	// the component's current first node goes to the front, any other to the back
	std::vector<uint64_t> comp_n(d.total_comp, 0);                // contours per component
	for (const Kept& k : kept) {
		if (k.comp >= d.ncomp_expect_host[k.zi]) throw Error(CKL_ERR_RUNTIME, "crackle_amd: point_cloud: component out of range");
		comp_n[comp_off[k.zi] + k.comp]++;
	}
	std::vector<uint64_t> comp_at(d.total_comp + 1, 0);
	for (uint64_t c = 0; c < d.total_comp; c++) comp_at[c + 1] = comp_at[c] + comp_n[c];
	std::vector<uint32_t> order(kept.size());                    // per component: its contours in merged order
	{
		std::vector<std::deque<uint32_t>> lists;                    // only for components with more than one contour
		std::vector<int64_t> list_of(d.total_comp, -1);
		for (uint32_t i = 0; i < kept.size(); i++) {
			const uint64_t c = comp_off[kept[i].zi] + kept[i].comp;
			if (comp_n[c] == 1) { order[comp_at[c]] = i; continue; }
			if (list_of[c] < 0) { list_of[c] = static_cast<int64_t>(lists.size()); lists.emplace_back(); }
			std::deque<uint32_t>& l = lists[list_of[c]];
			if (!l.empty() && kept[l.front()].first > kept[i].first) l.push_front(i);
			else l.push_back(i);
		}
		for (uint64_t c = 0; c < d.total_comp; c++) {
			if (list_of[c] < 0) continue;
			uint64_t at = comp_at[c];
			for (uint32_t i : lists[list_of[c]]) order[at++] = i;
		}
	}

	// operations.hpp:229-257: components in (z, index) order append to their label's points.  The
	// labels of the output are the table's entries that own a component of the range and pass the
	// filters, in table order
	std::vector<uint8_t> present(n_table, 0);
	for (uint64_t c = 0; c < d.total_comp; c++) {
		if (comp_key[c] >= n_table) throw Error(CKL_ERR_RUNTIME, "crackle_amd: point_cloud: a component's label is not in the stream's label table");
		present[comp_key[c]] = 1;
	}
	std::vector<int64_t> table_out(n_table, -1);
	std::vector<uint64_t> keys;
	for (uint32_t i = 0; i < n_table; i++) {
		const uint64_t label = d.stats_table[i] & lmask;
		if (!present[i] || !takes(label)) continue;
		table_out[i] = static_cast<int64_t>(keys.size());
		keys.push_back(label);
	}
	std::vector<uint64_t> off(keys.size() + 1, 0);
	std::vector<int64_t> key_of(d.total_comp, -1);
	for (uint64_t c = 0; c < d.total_comp; c++) {
		const int64_t k = table_out[comp_key[c]];
		if (k < 0) continue;
		key_of[c] = k;
		for (uint64_t j = comp_at[c]; j < comp_at[c + 1]; j++) off[k + 1] += kept[order[j]].len;
	}
	for (size_t k = 0; k < keys.size(); k++) off[k + 1] += off[k];
	const uint64_t total_points = off[keys.size()];
	out.labels = keys;
	out.offsets = off;
	out.points = host_out<uint16_t>(std::max<uint64_t>(total_points * 3, 1));
	if (!total_points) return;

	mark("order");
	DevBuf<uint16_t> d_points;
	d_points.ensure(total_points * 3);
	std::vector<uint64_t> fill(off.begin(), off.end() - 1);
	std::vector<std::vector<ContourJob>> jobs(chunks.size());
	{
		std::vector<uint32_t> chunk_of(ns);
		for (size_t ci = 0; ci < chunks.size(); ci++) for (uint32_t i = 0; i < chunks[ci].n; i++) chunk_of[chunks[ci].z0 + i] = static_cast<uint32_t>(ci);
		for (uint32_t zi = 0; zi < ns; zi++) {
			const Chunk& ch = chunks[chunk_of[zi]];
			for (uint64_t c = comp_off[zi]; c < comp_off[zi + 1]; c++) {
				if (key_of[c] < 0) continue;
				for (uint64_t j = comp_at[c]; j < comp_at[c + 1]; j++) {
					const Kept& k = kept[order[j]];
					ContourJob job;
					job.src = static_cast<uint64_t>(zi - ch.z0) * ch.raw_cap + k.offset;
					job.dst = fill[key_of[c]];
					job.len = k.len; job.rot = k.rot; job.z = static_cast<uint32_t>(d.z_start + zi); job.pad = 0;
					fill[key_of[c]] += k.len;
					jobs[chunk_of[zi]].push_back(job);
				}
			}
		}
	}
	mark("plan");
	DevBuf<ContourJob> d_jobs;
	for (size_t ci = 0; ci < chunks.size(); ci++) {
		if (jobs[ci].empty()) continue;
		upload(d_jobs, jobs[ci], s);
		const uint64_t nj = jobs[ci].size();
		hipLaunchKernelGGL(k_contour_emit, dim3(static_cast<uint32_t>((nj + 3) / 4)), dim3(256), 0, s, d_jobs.p, nj, chunks[ci].raw->p, h.sx, d_points.p);
		CKL_HIP(hipStreamSynchronize(s));      // the job list is reused by the next chunk
	}
	mark("emit");
	CKL_HIP(hipMemcpyAsync(out.points.get(), d_points.p, total_points * 6, hipMemcpyDeviceToHost, s));
	CKL_HIP(hipStreamSynchronize(s));
	CKL_HIP(hipGetLastError());
	mark("d2h");
	if (prof) fprintf(stderr, "[ckl point_cloud ms]%s | contours=%zu points=%llu walk_steps=%llu\n", marks.c_str(), kept.size(), static_cast<unsigned long long>(total_points), static_cast<unsigned long long>(walk_steps));
}

}  // namespace

namespace ckl {

// The box [x0, x1) x [y0, y1) of every slice of the session's range into a device buffer, dense
// (fortran_order streams: x fastest; others: z fastest), data_width bytes per voxel or one byte with
// has_label.  One pipeline run up to the run tables and the component -> label map, so a damaged slice
// of the range raises as for a decode wherever the box lies, then k_paint_window.
void decoder_cutout(ckl_decoder& d, int64_t x0, int64_t x1, int64_t y0, int64_t y1, void* out_device, uint64_t capacity, int has_label, uint64_t label) {
	const Header& h = d.head;
	check_box_axis("cutout", "x", x0, x1, h.sx);
	check_box_axis("cutout", "y", y0, y1, h.sy);
	const int ow = has_label ? 1 : h.data_width;
	const uint64_t wx = static_cast<uint64_t>(x1 - x0), wy = static_cast<uint64_t>(y1 - y0);
	const uint64_t need = wx * wy * d.nslices * static_cast<uint64_t>(ow);
	if (need == 0 || d.sxy == 0) return;
	if (!out_device || capacity < need) throw Error(CKL_ERR_ARG, "crackle_amd: output buffer too small: need " + std::to_string(need) + " bytes");
	decoder_run(d, { Goal::TABLES });
	hipStream_t s = d.stream;
	WindowArgs wa;
	wa.x0 = static_cast<uint32_t>(x0); wa.x1 = static_cast<uint32_t>(x1); wa.y0 = static_cast<uint32_t>(y0); wa.y1 = static_cast<uint32_t>(y1);
	wa.rows = static_cast<uint32_t>(std::min<uint64_t>(std::min<uint64_t>(kWinRows, wy), std::max<uint64_t>(1, kWinTile / wx)));
	wa.nslices = d.nslices;
	wa.fortran_order = h.fortran_order ? 1u : 0u;
	wa.has_label = has_label ? 1u : 0u; wa.label = label;
	const dim3 grid(static_cast<uint32_t>((wy + wa.rows - 1) / wa.rows), d.nslices);
	// the paint as one more stage of the run's table (ckl_decoder_stage_timing), between two events of its own:
	// the pipeline's last event lies before the host has read the slices' verdicts
	const int st = d.n_stages;
	const bool timed = d.stage_events && st + 2 <= kMaxStages;
	if (timed) CKL_HIP(hipEventRecord(d.ev[st + 1], s));
	with_label_type(ow, [&](auto t) {
		typedef typename decltype(t)::type OUT;
		hipLaunchKernelGGL(k_paint_window<OUT>, grid, dim3(kBlock), 0, s, run_geom(d), run_arrays(d), d.d_label_map.p, d.d_comp_off.p, d.d_ncomp_expect.p, wa, reinterpret_cast<OUT*>(out_device));
	});
	if (timed) CKL_HIP(hipEventRecord(d.ev[st + 2], s));
	record_span(d);
	CKL_HIP(hipGetLastError());
	if (timed) {
		CKL_HIP(hipEventElapsedTime(&d.stage_ms[st], d.ev[st + 1], d.ev[st + 2]));
		d.stage_name[st] = "k_paint_window";
		d.n_stages = st + 1;
	}
}

}  // namespace ckl

extern "C" {

int ckl_decoder_cutout(ckl_decoder* d, int64_t x0, int64_t x1, int64_t y0, int64_t y1, void* out_device, uint64_t out_capacity_bytes, int has_label, uint64_t label) {
	return guard([&] {
		enter(d);
		decoder_cutout(*d, x0, x1, y0, y1, out_device, out_capacity_bytes, has_label, label);
	});
}

int ckl_cutout(
	const uint8_t* buf, uint64_t n, void* out, uint64_t out_capacity_bytes, int out_mem,
	int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1,
	int has_label, uint64_t label, int device
) {
	return guard([&]() -> int {
		if (!buf) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		const Header h = Header::parse(buf, n);
		check_box_axis("cutout", "x", x0, x1, h.sx);
		check_box_axis("cutout", "y", y0, y1, h.sy);
		check_box_axis("cutout", "z", z0, z1, h.sz);
		const uint64_t need = static_cast<uint64_t>(x1 - x0) * static_cast<uint64_t>(y1 - y0) * static_cast<uint64_t>(z1 - z0) * static_cast<uint64_t>(has_label ? 1 : h.data_width);
		if (need == 0) return CKL_OK;
		if (!out || out_capacity_bytes < need) throw Error(CKL_ERR_ARG, "crackle_amd: output buffer too small: need " + std::to_string(need) + " bytes");
		// whole planes: the decode itself, which keeps the strip kernels
		if (x0 == 0 && x1 == h.sx && y0 == 0 && y1 == h.sy) return ckl_decompress(buf, n, out, out_capacity_bytes, out_mem, z0, z1, has_label, label, device);
		DecoderPtr d;
		const int rc = open_decoder(buf, n, z0, z1, device, d);
		if (rc != CKL_OK) return rc;
		if (out_mem == CKL_MEM_DEVICE) {
			enter(d.get());
			decoder_cutout(*d, x0, x1, y0, y1, out, out_capacity_bytes, has_label, label);
		}
		else {
			DevBuf<uint8_t> tmp;      // the box alone, on the card and over the link
			tmp.ensure(need);
			decoder_cutout(*d, x0, x1, y0, y1, tmp.p, need, has_label, label);
			CKL_HIP(hipMemcpy(out, tmp.p, need, hipMemcpyDeviceToHost));
		}
		return CKL_OK;
	});
}

int ckl_decoder_label_stats(ckl_decoder* d, uint64_t capacity, uint64_t* labels, uint64_t* counts, uint64_t* sums, uint32_t* boxes, uint64_t* n_labels) {
	return guard([&] {
		if (!d || !n_labels) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		enter(d);
		decoder_label_stats(*d, capacity, labels, counts, sums, boxes, n_labels);
	});
}

int ckl_decoder_contacts(ckl_decoder* d, uint64_t** pairs, uint64_t** faces, uint64_t* n_pairs) {
	return guard([&] {
		if (!d || !pairs || !faces || !n_pairs) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		*pairs = nullptr; *faces = nullptr; *n_pairs = 0;
		enter(d);
		std::vector<uint64_t> p, f;
		decoder_contacts(*d, p, f);
		const uint64_t n = p.size() / 2;
		auto po = host_out<uint64_t>(std::max<uint64_t>(2 * n, 1)), fo = host_out<uint64_t>(std::max<uint64_t>(3 * n, 1));
		if (n) { memcpy(po.get(), p.data(), 2 * n * 8); memcpy(fo.get(), f.data(), 3 * n * 8); }
		*pairs = po.release(); *faces = fo.release(); *n_pairs = n;
	});
}

// the table of decoder_overlaps handed to the caller (a block of one element each when it is empty)
static void overlaps_out(OverlapTable& t, uint64_t** pairs, uint64_t** counts, uint64_t* n_pairs) {
	if (!t.pairs) t.pairs = host_out<uint64_t>(1);
	if (!t.counts) t.counts = host_out<uint64_t>(1);
	*pairs = t.pairs.release(); *counts = t.counts.release(); *n_pairs = t.n;
}

int ckl_decoder_overlaps(ckl_decoder* a, ckl_decoder* b, uint64_t** pairs, uint64_t** counts, uint64_t* n_pairs) {
	return guard([&] {
		if (!a || !b || !pairs || !counts || !n_pairs) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		*pairs = nullptr; *counts = nullptr; *n_pairs = 0;
		OverlapTable t;
		enter(b);
		enter(a);
		decoder_overlaps(*a, *b, t);
		overlaps_out(t, pairs, counts, n_pairs);
	});
}

int ckl_overlaps(
	const uint8_t* buf1, uint64_t n1, const uint8_t* buf2, uint64_t n2,
	int64_t z_start, int64_t z_end, int device, uint64_t** pairs, uint64_t** counts, uint64_t* n_pairs
) {
	return guard([&]() -> int {
		if (!buf1 || !buf2 || !pairs || !counts || !n_pairs) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		*pairs = nullptr; *counts = nullptr; *n_pairs = 0;
		const Header h1 = Header::parse(buf1, n1), h2 = Header::parse(buf2, n2);
		// from the two headers alone, before a device is touched
		if (h1.sx != h2.sx || h1.sy != h2.sy || h1.sz != h2.sz)
			throw Error(CKL_ERR_ARG, "crackle_amd: overlaps: the volumes differ in shape: " + std::to_string(h1.sx) + " x " + std::to_string(h1.sy) + " x " + std::to_string(h1.sz)
				+ " and " + std::to_string(h2.sx) + " x " + std::to_string(h2.sy) + " x " + std::to_string(h2.sz));
		int64_t zs, ze;
		clamp_range(h1, z_start, z_end, zs, ze);
		OverlapTable t;
		if (static_cast<uint64_t>(h1.sx) * h1.sy != 0) {
			DecoderPtr d1, d2;
			int rc = open_decoder(buf1, n1, zs, ze, device, d1);
			if (rc == CKL_OK) rc = open_decoder(buf2, n2, zs, ze, device, d2);
			if (rc != CKL_OK) return rc;
			decoder_overlaps(*d1, *d2, t);
		}
		overlaps_out(t, pairs, counts, n_pairs);
		return CKL_OK;
	});
}

int ckl_connected_components(
	const uint8_t* buf, uint64_t n, int connectivity, int device,
	uint8_t** out, uint64_t* out_len, uint64_t** component_labels, uint64_t* n_components
) {
	return guard([&]() -> int {
		if (!buf || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		*out = nullptr; *out_len = 0;
		if (component_labels) *component_labels = nullptr;
		if (n_components) *n_components = 0;
		if (connectivity != 6 && connectivity != 18 && connectivity != 26) throw Error(CKL_ERR_ARG, "crackle_amd: connected_components: connectivity must be 6, 18 or 26");
		const Header h = Header::parse(buf, n);
		if (h.format_version != 1) throw Error(CKL_ERR_ARG, "crackle_amd: connected components need a version 1 stream: version 0 has no crack crcs to carry over");
		Components3D cc;
		std::vector<uint64_t> uniq;
		if (h.voxels() != 0) {      // (an empty volume: its header, from the host alone)
			DecoderPtr d;
			const int rc = open_decoder(buf, n, 0, -1, device, d);
			if (rc != CKL_OK) return rc;
			enter(d.get());
			decoder_connected_components(*d, connectivity, component_labels != nullptr, cc);
			uniq.resize(cc.n_components + (cc.has_zero ? 1 : 0));
			for (uint64_t i = 0; i < uniq.size(); i++) uniq[i] = i + (cc.has_zero ? 0 : 1);
		}
		HostOut<uint64_t> lo;
		if (component_labels) {
			lo = host_out<uint64_t>(std::max<uint64_t>(cc.n_components, 1));
			if (cc.n_components) memcpy(lo.get(), cc.root_labels.data(), cc.n_components * 8);
		}
		*out = relabel_stream(buf, n, uniq, cc.keys.data(), cc.key_width, cc.keys.size() / cc.key_width, out_len);
		if (component_labels) *component_labels = lo.release();
		if (n_components) *n_components = cc.n_components;
		return CKL_OK;
	});
}

int ckl_dust(
	const uint8_t* buf, uint64_t n, uint64_t threshold, int connectivity, int flags, int device,
	uint8_t** out, uint64_t* out_len, uint64_t* n_removed
) {
	return guard([&]() -> int {
		if (!buf || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		*out = nullptr; *out_len = 0;
		if (n_removed) *n_removed = 0;
		if (connectivity != 6 && connectivity != 18 && connectivity != 26) throw Error(CKL_ERR_ARG, "crackle_amd: dust: connectivity must be 6, 18 or 26");
		if (flags & ~(CKL_DUST_BINARY_IMAGE | CKL_DUST_INVERT)) throw Error(CKL_ERR_ARG, "crackle_amd: dust: unknown flags");
		const Header h = Header::parse(buf, n);
		if (h.format_version != 1) throw Error(CKL_ERR_ARG, "crackle_amd: dust: version 0 streams have no crack crcs to carry over: recompress() first");
		if (h.is_signed) throw Error(CKL_ERR_ARG, "crackle_amd: dust: signed streams are not supported");
		LabelEdit du;
		if (h.voxels() != 0) {      // (an empty volume comes back as it is, from the host alone)
			DecoderPtr d;
			const int rc = open_decoder(buf, n, 0, -1, device, d);
			if (rc != CKL_OK) return rc;
			enter(d.get());
			decoder_dust(*d, threshold, connectivity, (flags & CKL_DUST_BINARY_IMAGE) != 0, (flags & CKL_DUST_INVERT) != 0, du);
		}
		*out = relabel_stream_keep_width(buf, n, du.uniq, du.keys.data(), du.key_width, du.keys.size() / du.key_width, out_len);
		if (n_removed) *n_removed = du.n_changed;
		return CKL_OK;
	});
}

int ckl_fill_holes(
	const uint8_t* buf, uint64_t n, int connectivity, int device,
	uint8_t** out, uint64_t* out_len, uint64_t* n_filled
) {
	return guard([&]() -> int {
		if (!buf || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		*out = nullptr; *out_len = 0;
		if (n_filled) *n_filled = 0;
		if (connectivity != 6 && connectivity != 18 && connectivity != 26) throw Error(CKL_ERR_ARG, "crackle_amd: fill_holes: connectivity must be 6, 18 or 26");
		const Header h = Header::parse(buf, n);
		if (h.format_version != 1) throw Error(CKL_ERR_ARG, "crackle_amd: fill_holes: version 0 streams have no crack crcs to carry over: recompress() first");
		if (h.is_signed) throw Error(CKL_ERR_ARG, "crackle_amd: fill_holes: signed streams are not supported");
		LabelEdit fh;
		if (h.voxels() != 0) {      // (an empty volume comes back as it is, from the host alone)
			DecoderPtr d;
			const int rc = open_decoder(buf, n, 0, -1, device, d);
			if (rc != CKL_OK) return rc;
			enter(d.get());
			decoder_fill_holes(*d, connectivity, fh);
		}
		*out = relabel_stream_keep_width(buf, n, fh.uniq, fh.keys.data(), fh.key_width, fh.keys.size() / fh.key_width, out_len);
		if (n_filled) *n_filled = fh.n_changed;
		return CKL_OK;
	});
}

int ckl_decoder_vcg(ckl_decoder* d, uint8_t* out_device, uint64_t out_capacity_bytes, int connectivity) {
	return guard([&] {
		enter(d);
		decoder_vcg(*d, out_device, out_capacity_bytes, connectivity);
	});
}

int ckl_voxel_connectivity_graph(const uint8_t* buf, uint64_t n, int connectivity, int device, uint8_t* out_host, uint64_t out_capacity_bytes) {
	return ckl_voxel_connectivity_graph_range(buf, n, 0, -1, connectivity, device, out_host, out_capacity_bytes);
}

int ckl_voxel_connectivity_graph_range(const uint8_t* buf, uint64_t n, int64_t z_start, int64_t z_end, int connectivity, int device, uint8_t* out_host, uint64_t out_capacity_bytes) {
	DecoderPtr d;
	const int rc = open_decoder(buf, n, z_start, z_end, device, d);
	if (rc != CKL_OK) return rc;
	return guard([&] {
		const uint64_t need = d->sxy * d->nslices;
		if (need) {
			if (!out_host || out_capacity_bytes < need) throw Error(CKL_ERR_ARG, "crackle_amd: output buffer too small: need " + std::to_string(need) + " bytes");
			DevBuf<uint8_t> tmp;
			tmp.ensure(need);
			decoder_vcg(*d, tmp.p, need, connectivity);
			CKL_HIP(hipMemcpy(out_host, tmp.p, need, hipMemcpyDeviceToHost));
		}
		else if (connectivity != 4 && connectivity != 6) throw Error(CKL_ERR_ARG, "crackle: voxel_connectivity_graph: only connectivity 4 and 6 are currently supported.");
	});
}

int ckl_point_cloud(
	const uint8_t* buf, uint64_t n, int64_t z_start, int64_t z_end,
	const uint64_t* labels, uint64_t n_labels, int has_labels, int skip_background, int device,
	uint64_t** labels_out, uint64_t** offsets_out, uint16_t** points_out, uint64_t* n_out
) {
	return guard([&]() -> int {
		if (!buf || !labels_out || !offsets_out || !points_out || !n_out || (has_labels && n_labels && !labels)) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		*labels_out = nullptr; *offsets_out = nullptr; *points_out = nullptr; *n_out = 0;
		const Header h = Header::parse(buf, n);
		int64_t zs, ze;
		clamp_range(h, z_start, z_end, zs, ze);
		DecoderPtr d;
		const int rc = open_decoder(buf, n, zs, ze, device, d);
		if (rc != CKL_OK) return rc;
		PointCloud pc;
		decoder_point_cloud(*d, labels, n_labels, has_labels != 0, skip_background != 0, pc);
		const uint64_t k = pc.labels.size();
		auto lo = host_out<uint64_t>(std::max<uint64_t>(k, 1)), oo = host_out<uint64_t>(k + 1);
		if (k) memcpy(lo.get(), pc.labels.data(), k * 8);
		memcpy(oo.get(), pc.offsets.data(), (k + 1) * 8);
		if (!pc.points) pc.points = host_out<uint16_t>(1);
		*labels_out = lo.release(); *offsets_out = oo.release(); *points_out = pc.points.release(); *n_out = k;
		return CKL_OK;
	});
}

int ckl_array_equal(const uint8_t* buf1, uint64_t n1, const uint8_t* buf2, uint64_t n2, int device, int* equal) {
	return guard([&]() -> int {
		if (!buf1 || !buf2 || !equal) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		*equal = 0;
		const Header h1 = Header::parse(buf1, n1), h2 = Header::parse(buf2, n2);
		// operations.hpp:1049-1062; get_voxels -> get_szr (:54-87) throws for a stream without slices
		if (h1.sz == 0 || h2.sz == 0) throw Error(CKL_ERR_RUNTIME, "crackle: Invalid range: 0 - 0");
		if (h1.voxels() == 0 || h2.voxels() == 0) { *equal = h1.voxels() == h2.voxels(); return CKL_OK; }
		if (h1.sx != h2.sx || h1.sy != h2.sy || h1.sz != h2.sz) return CKL_OK;
		DecoderPtr d1, d2;
		int rc = open_decoder(buf1, n1, 0, -1, device, d1);
		if (rc == CKL_OK) rc = open_decoder(buf2, n2, 0, -1, device, d2);
		if (rc != CKL_OK) return rc;
		// the reference compares the component counts its CCL finds (:1146-1149); those of a valid
		// stream are the counts its label section states
		if (d1->ncomp_expect_host != d2->ncomp_expect_host) return CKL_OK;
		// label_map1[ccl1] against label_map1[ccl2] (:1160-1171; yes, label_map1 on both sides): the
		// first stream is decoded as it is, the second one's components are painted through the FIRST
		// stream's component -> label table.  Both x fastest, whatever the headers say.
		d1->use_general = true; d2->use_general = true;      // the general pipeline keeps the component -> label table
		d1->head.fortran_order = true; d2->head.fortran_order = true;
		const uint64_t bytes = d1->sxy * d1->nslices * static_cast<uint64_t>(h1.data_width);
		DevBuf<uint8_t> a, b;
		DevBuf<uint32_t> flag;
		a.ensure(bytes); b.ensure(bytes); flag.ensure(1);
		decoder_run(*d1, { Goal::PAINT, a.p, bytes });
		d2->foreign_label_map = d1->d_label_map.p;
		d2->paint_width = h1.data_width;
		CKL_HIP(hipStreamSynchronize(d1->stream));
		decoder_run(*d2, { Goal::PAINT, b.p, bytes });
		hipStream_t s = d2->stream;
		CKL_HIP(hipMemsetAsync(flag.p, 0, sizeof(uint32_t), s));
		hipLaunchKernelGGL(k_buffers_differ, dim3(2048), dim3(kBlock), 0, s, a.p, b.p, bytes, flag.p);
		uint32_t differ = 0;
		CKL_HIP(hipMemcpyAsync(&differ, flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
		CKL_HIP(hipStreamSynchronize(s));
		CKL_HIP(hipGetLastError());
		*equal = differ ? 0 : 1;
		return CKL_OK;
	});
}

int ckl_mode_pooling_2x2x1(
	const uint8_t* buf, uint64_t n, int64_t z_start, int64_t z_end, int device,
	uint8_t** out, uint64_t* out_len, uint64_t** lengths, uint64_t* count
) {
	return guard([&]() -> int {
		if (!buf || !out || !out_len || !lengths || !count) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		*out = nullptr; *out_len = 0; *lengths = nullptr; *count = 0;
		const Header h = Header::parse(buf, n);
		// an empty range is an error, an empty slice is not (operations.hpp:1213-1215)
		int64_t zs, ze;
		clamp_range(h, z_start, z_end, zs, ze);
		if (static_cast<uint64_t>(h.sx) * h.sy == 0) return CKL_OK;
		DecoderPtr d;
		int rc = open_decoder(buf, n, z_start < 0 ? 0 : z_start, z_end, device, d);
		if (rc != CKL_OK) return rc;
		d->head.fortran_order = true;      // the pooling walks x fastest (operations.hpp:1241-1249)
		d->use_general = d->use_general || !(h.fortran_order);      // a C-order stream was laid out for the general pipeline
		const uint32_t sx = h.sx, sy = h.sy, nz = d->nslices;
		const uint32_t osx = (sx + 1u) >> 1, osy = (sy + 1u) >> 1;
		const int w = h.data_width;
		const uint64_t vox = d->sxy * nz, ovox = static_cast<uint64_t>(osx) * osy * nz;
		DevBuf<uint8_t> full, pooled;
		full.ensure(vox * w); pooled.ensure(ovox * w);
		decoder_run(*d, { Goal::PAINT, full.p, vox * w });
		hipStream_t s = d->stream;
		const dim3 grid(static_cast<uint32_t>((ovox + kBlock - 1) / kBlock));
		with_label_type(w, [&](auto t) {
			typedef typename decltype(t)::type LABEL;
			hipLaunchKernelGGL(k_mode_pool_2x2<LABEL>, grid, dim3(kBlock), 0, s, reinterpret_cast<const LABEL*>(full.p), reinterpret_cast<LABEL*>(pooled.p), sx, sy, nz);
		});
		CKL_HIP(hipStreamSynchronize(s));
		CKL_HIP(hipGetLastError());
		// every pooled slice becomes a stream of its own: crackle::compress<LABEL>(oimg, osx, osy, 1) with
		// its defaults (operations.hpp:1294-1297; LABEL is the unsigned type of the data width)
		ckl_encoder* enc = nullptr;
		rc = ckl_encoder_create(osx, osy, 1, w, device, &enc);
		if (rc != CKL_OK) return rc;
		EncoderPtr e(enc);
		std::vector<uint8_t> all;
		auto lens = host_out<uint64_t>(nz ? nz : 1);
		for (uint32_t z = 0; z < nz; z++) {
			uint8_t* one = nullptr; uint64_t len = 0;
			rc = ckl_encoder_run(e.get(), pooled.p + static_cast<uint64_t>(z) * osx * osy * w, osx, osy, 1, 0, 1, 0, 0, 1, 0, nullptr, &one, &len);
			if (rc != CKL_OK) return rc;
			all.insert(all.end(), one, one + len);
			lens[z] = len;
			ckl_free(one);
		}
		e.reset();
		d.reset();
		uint8_t* o = static_cast<uint8_t*>(host_out_alloc(all.size() ? all.size() : 1));
		memcpy(o, all.data(), all.size());
		*out = o; *out_len = all.size(); *lengths = lens.release(); *count = nz;
		return CKL_OK;
	});
}

}  // extern "C"
