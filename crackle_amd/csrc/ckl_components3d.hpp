// 3D connected components from the run tables: the device half of connected_components, of dust and of
// fill_holes (whose own kernels, k_cc_voxels / k_hole_scan / k_edit_mark / k_edit_keys, stand at the end).
// (Included by ckl_operations.hip inside namespace ckl, after the contacts kernels whose run walk and
// constants it shares: kContactBlock / kContactPer / kContactRuns, kNoKey.)
//
// The crack codes of a slice already describe its 4-connected components, and the decoder numbers
// them in the order of their first raster pixel.  A 3D component of a label is a union of those 2D
// components: nothing has to be painted, the components only have to be LINKED wherever two of them
// with the same label hold neighbouring voxels, and the sets numbered.
//
//   k_cc_init      parent[c] = c over the global component ids (slice offset + id in the slice)
//   k_run_links    one run per thread (the layout of k_run_contacts): the runs of the neighbouring
//                  rows are walked through word_base and the vertical-crack plane; where the label
//                  is the same and is not 0 the two components are united (LinkArgs::mode: or any two
//                  foreground components, or the components of label 0 and no others).
//   k_cc_flatten   root of every component (its set's smallest id)
//   k_cc_count / k_cc_offsets / k_cc_number
//                  device-wide exclusive scan over the roots with a nonzero label: a root's number
//                  is 1 + its rank.  Global ids ascend with (z, first raster pixel), so a set's
//                  smallest id belongs to the component that holds the set's first voxel in
//                  x-fastest, then y, then z order, and the ranks of the roots are the numbering by
//                  first voxel.
//   k_cc_keys      every component's key into the new unique list, packed at the key width
//
// Rows and x ranges looked at from the run [x0, x1] of row y in slice z (clamped to the slice):
//
//   connectivity   same slice                              previous slice
//   6              next run of the row; row y-1 [x0, x1]     row y [x0, x1]
//   18             next run; row y-1 [x0-1, x1+1]            row y [x0-1, x1+1]; rows y-1, y+1 [x0, x1]
//   26             as 18                                     rows y-1, y, y+1 [x0-1, x1+1]
//
// The later run of every neighbouring pair does the looking (rows above, the slice before), so each
// pair is seen once.  In the same slice two different components with one label only exist in a
// stream whose label table was rewritten without re-encoding; they are united too.
//
// Union-find without locks: parents only ever decrease.  unite() hooks the larger of two roots
// under the smaller with atomicMin and goes on with the value it displaced, so whatever the order in
// which the atomics land, a set's root ends up as its smallest member: the result does not depend on
// scheduling.
#pragma once

enum : uint32_t { CC_BADKEY = 0, CC_HAS_ZERO = 1, CC_COUNT = 2, CC_FLAGS = 4 };

// What k_run_links unites: neighbouring components of one nonzero label; any two neighbouring foreground
// components, whatever their labels (dust's binary_image); or the components of label 0 alone (fill_holes),
// which the other two never touch.
enum : uint32_t { LINK_BY_LABEL = 0, LINK_FOREGROUND = 1, LINK_BACKGROUND = 2 };

struct LinkArgs {
	const uint32_t* comp_key;        // [total_comp] label table index of every component (kNoKey: not in the table)
	uint32_t zero_key;               // table index of label 0 (kNoKey: absent): background, linked in LINK_BACKGROUND alone
	uint32_t sx, sy, n_pixels;
	uint32_t connectivity;           // 6, 18 or 26
	uint32_t mode;                   // LINK_BY_LABEL, LINK_FOREGROUND or LINK_BACKGROUND
	uint32_t* parent;                // [total_comp]
	uint32_t* flags;                 // [CC_FLAGS]
};

__device__ __forceinline__ uint32_t cc_parent(const uint32_t* parent, uint32_t x) {
	return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t cc_find(const uint32_t* parent, uint32_t x) {
	for (;;) {
		const uint32_t p = cc_parent(parent, x);
		if (p == x) return x;
		x = p;
	}
}

// An ancestor of x from ordinary (cached) loads.  A value read late is still a value parent[x] once
// held, and whatever x pointed at stays in x's set: the walk ends at a member of the set at or above
// the root it would have found then, and cc_unite goes on from there with loads that see the atomics.
__device__ __forceinline__ uint32_t cc_walk_cached(const uint32_t* parent, uint32_t x) {
	for (;;) {
		const uint32_t p = parent[x];
		if (p == x) return x;
		x = p;
	}
}

// unites the sets of a and b; a (the caller's stand-in for its own component) becomes the root found,
// so that the thread's next link starts where this one ended
__device__ __forceinline__ void cc_unite(uint32_t* parent, uint32_t& a, uint32_t b) {
	a = cc_walk_cached(parent, a);
	b = cc_walk_cached(parent, b);
	while (a != b) {
		a = cc_find(parent, a);
		b = cc_find(parent, b);
		if (a == b) break;
		if (a < b) { const uint32_t t = a; a = b; b = t; }
		// a > b: hook a under b.  A displaced parent other than a itself means somebody hooked a in
		// the meantime: a now points at min(old, b), and old and b are still to be united.
		const uint32_t old = atomicMin(parent + a, b);
		if (old == a) { a = b; break; }
		a = old;
	}
}

// are a component of label index ka (one that the mode links: label 0's in LINK_BACKGROUND and only there) and a
// neighbouring one of label index kb one piece?  (LINK_BACKGROUND: ka is zero_key, so "the same label" says
// that the other one is label 0 too)
__device__ __forceinline__ bool cc_joined(const LinkArgs& la, uint32_t ka, uint32_t kb) {
	return la.mode == LINK_FOREGROUND ? kb != la.zero_key : kb == ka;
}

// The runs of row y of slice zj that hold pixels of [lo, hi], in order: visit(component of the run).  The first
// one comes from word_base and the break words, the others follow it in the run arrays.  false: the run tables
// do not cover the row.
template <typename Visit>
__device__ __forceinline__ bool walk_row(
	const RunGeom& g, const RunArrays& r, uint32_t sx, uint32_t n_pixels, uint32_t zj, uint32_t y, uint32_t lo, uint32_t hi, Visit&& visit
) {
	const uint64_t rb = r.rbase[zj];
	const uint32_t nj = r.nruns[zj];
	const uint32_t row = y * sx;
	const uint32_t w = lo >> 5;
	uint32_t j = r.word_base[zj * g.plane_words + y * g.row_words + w] + __popc(g.breaks(zj, y, w) & mask_le(lo & 31u)) - 1u;
	while (j < nj) {
		// the run after the last one of a row starts the next row (or the slice ends): e <= sx
		const uint32_t e = (j + 1 < nj ? r.run_start[rb + j + 1] : n_pixels) - row;
		visit(r.run_cc[rb + j]);
		if (e > hi) return true;
		j++;
	}
	return false;
}

// links between the run's pixels [lo, hi] (a member ga of its component's set, label index ka) and the runs of row
// y of slice zj; skip: the run's own component where zj is its slice (kNoKey otherwise)
__device__ __forceinline__ void link_row(
	const RunGeom& g, const RunArrays& r, const LinkArgs& la,
	uint32_t zj, const uint32_t* key_j, uint32_t nce_j, uint32_t off_j, uint32_t y, uint32_t lo, uint32_t hi,
	uint32_t skip, uint32_t& ga, uint32_t ka, uint32_t& last
) {
	const bool covered = walk_row(g, r, la.sx, la.n_pixels, zj, y, lo, hi, [&](uint32_t ccj) {
		if (ccj == skip) return;
		const uint32_t kj = ccj < nce_j ? key_j[ccj] : kNoKey;
		if (kj == kNoKey) atomicOr(la.flags + CC_BADKEY, 1u);
		else if (cc_joined(la, ka, kj) && off_j + ccj != last) {
			last = off_j + ccj;
			cc_unite(la.parent, ga, last);
		}
	});
	if (!covered) atomicOr(la.flags + CC_BADKEY, 1u);
}

// grid = (ceil(most runs of a slice / kContactRuns), nslices), block = kContactBlock
static __global__ void __launch_bounds__(kContactBlock) k_run_links(
	RunGeom g, RunArrays r, const uint64_t* __restrict__ comp_off, const uint32_t* __restrict__ ncomp_expect, LinkArgs la
) {
	const uint32_t zi = blockIdx.y;
	const uint32_t n = r.nruns[zi];
	const uint32_t i0 = blockIdx.x * kContactRuns;
	if (i0 >= n) return;
	const uint64_t rb = r.rbase[zi];
	const uint32_t nce = ncomp_expect[zi];
	const uint32_t off = static_cast<uint32_t>(comp_off[zi]);
	const uint32_t* key_z = la.comp_key + off;
	const uint32_t nce_p = zi ? ncomp_expect[zi - 1] : 0u;
	const uint32_t off_p = zi ? static_cast<uint32_t>(comp_off[zi - 1]) : 0u;
	const uint32_t* key_p = la.comp_key + off_p;
	const bool diag = la.connectivity != 6;
	const bool corners = la.connectivity == 26;
	for (uint32_t k = 0; k < kContactPer; k++) {
		const uint32_t i = i0 + k * kContactBlock + threadIdx.x;
		if (i >= n) break;
		const uint32_t a = r.run_start[rb + i];
		const uint32_t b = i + 1 < n ? r.run_start[rb + i + 1] : la.n_pixels;
		const uint32_t cc = r.run_cc[rb + i];
		const uint32_t y = a / la.sx;
		const uint32_t row = y * la.sx;
		const uint32_t x0 = a - row, x1 = b - 1 - row;
		const uint32_t ka = cc < nce ? key_z[cc] : kNoKey;
		if (ka == kNoKey) { atomicOr(la.flags + CC_BADKEY, 1u); continue; }
		if ((ka == la.zero_key) != (la.mode == LINK_BACKGROUND)) continue;      // label 0's runs in that mode alone, and no others there
		uint32_t ga = off + cc;      // the component, then the highest member of its set that a link has found
		uint32_t last = ga;          // the component of the link this thread made last: the same again is skipped
		if (b < row + la.sx) {      // the next run is in the same row
			const uint32_t cc2 = r.run_cc[rb + i + 1];
			if (cc2 != cc) {
				const uint32_t kb = cc2 < nce ? key_z[cc2] : kNoKey;
				if (kb == kNoKey) atomicOr(la.flags + CC_BADKEY, 1u);
				else if (cc_joined(la, ka, kb)) { last = off + cc2; cc_unite(la.parent, ga, last); }
			}
		}
		const uint32_t xl = x0 ? x0 - 1 : 0u, xr = min(x1 + 1, la.sx - 1);      // [x0 - 1, x1 + 1] inside the slice
		if (y > 0) link_row(g, r, la, zi, key_z, nce, off, y - 1, diag ? xl : x0, diag ? xr : x1, cc, ga, ka, last);
		if (zi == 0) continue;
		link_row(g, r, la, zi - 1, key_p, nce_p, off_p, y, diag ? xl : x0, diag ? xr : x1, kNoKey, ga, ka, last);
		if (!diag) continue;
		if (y > 0) link_row(g, r, la, zi - 1, key_p, nce_p, off_p, y - 1, corners ? xl : x0, corners ? xr : x1, kNoKey, ga, ka, last);
		if (y + 1 < la.sy) link_row(g, r, la, zi - 1, key_p, nce_p, off_p, y + 1, corners ? xl : x0, corners ? xr : x1, kNoKey, ga, ka, last);
	}
}

static __global__ void __launch_bounds__(kBlock) k_cc_init(uint32_t* __restrict__ parent, uint32_t n) {
	const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
	if (c < n) parent[c] = c;
}

// root[c] = the smallest id of c's set (parent is read only: nothing moves under the walk)
static __global__ void __launch_bounds__(kBlock) k_cc_flatten(const uint32_t* __restrict__ parent, uint32_t n, uint32_t* __restrict__ root) {
	const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
	if (c >= n) return;
	uint32_t x = c, p = parent[c];
	while (p != x) { x = p; p = parent[x]; }
	root[c] = x;
}

// The scan over the numbered roots, kCcPer components per thread: counts per workgroup, their
// exclusive prefix (one workgroup), then the numbers.
constexpr uint32_t kCcPer = 4;
constexpr uint32_t kCcTile = kBlock * kCcPer;

__device__ __forceinline__ uint32_t cc_numbered(const uint32_t* root, const uint32_t* comp_key, uint32_t zero_key, uint32_t c, uint32_t n) {
	return (c < n && root[c] == c && comp_key[c] != zero_key) ? 1u : 0u;
}

static __global__ void __launch_bounds__(kBlock) k_cc_count(
	const uint32_t* __restrict__ root, const uint32_t* __restrict__ comp_key, uint32_t zero_key, uint32_t n,
	uint32_t* __restrict__ blk, uint32_t* __restrict__ flags
) {
	__shared__ uint32_t s_red[kWaves];
	const uint32_t c0 = blockIdx.x * kCcTile + threadIdx.x * kCcPer;
	uint32_t cnt = 0, zero = 0;
#pragma unroll
	for (uint32_t j = 0; j < kCcPer; j++) {
		cnt += cc_numbered(root, comp_key, zero_key, c0 + j, n);
		zero |= (c0 + j < n && comp_key[c0 + j] == zero_key) ? 1u : 0u;
	}
	if (zero) atomicOr(flags + CC_HAS_ZERO, 1u);
	cnt = block_sum(cnt, s_red);
	if (threadIdx.x == 0) blk[blockIdx.x] = cnt;
}

// grid = 1
static __global__ void __launch_bounds__(kBlock) k_cc_offsets(uint32_t* __restrict__ blk, uint32_t nb, uint32_t* __restrict__ flags) {
	__shared__ uint32_t s_scan[kWaves];
	uint32_t carry = 0;
	for (uint32_t b0 = 0; b0 < nb; b0 += kBlock) {
		const uint32_t b = b0 + threadIdx.x;
		uint32_t v[1] = { b < nb ? blk[b] : 0u }, tot[1];
		block_excl_add<1>(v, tot, s_scan);
		if (b < nb) blk[b] = carry + v[0];
		carry += tot[0];
	}
	if (threadIdx.x == 0) flags[CC_COUNT] = carry;
}

// number[c] = 1 + rank for the numbered roots (others are not written); root_label[rank] = the root's label
static __global__ void __launch_bounds__(kBlock) k_cc_number(
	const uint32_t* __restrict__ root, const uint32_t* __restrict__ comp_key, uint32_t zero_key, uint32_t n,
	const uint32_t* __restrict__ blk, uint32_t* __restrict__ number,
	const uint64_t* __restrict__ label_map, uint64_t* __restrict__ root_label
) {
	__shared__ uint32_t s_scan[kWaves];
	const uint32_t c0 = blockIdx.x * kCcTile + threadIdx.x * kCcPer;
	uint32_t f[kCcPer], v[1] = { 0 }, tot[1];
#pragma unroll
	for (uint32_t j = 0; j < kCcPer; j++) {
		f[j] = cc_numbered(root, comp_key, zero_key, c0 + j, n);
		v[0] += f[j];
	}
	block_excl_add<1>(v, tot, s_scan);
	uint32_t at = blk[blockIdx.x] + v[0];
#pragma unroll
	for (uint32_t j = 0; j < kCcPer; j++) {
		if (!f[j]) continue;
		if (root_label) root_label[at] = label_map[c0 + j];
		number[c0 + j] = ++at;
	}
}

// keys[c] = index of c's new value in the unique list (0, 1 .. N with a zero label somewhere, else
// 1 .. N), at the width of the list's length: four components per thread, one store
static __global__ void __launch_bounds__(kBlock) k_cc_keys(
	const uint32_t* __restrict__ root, const uint32_t* __restrict__ comp_key, uint32_t zero_key, uint32_t n,
	const uint32_t* __restrict__ number, const uint32_t* __restrict__ flags, uint8_t* __restrict__ keys
) {
	static_assert(kCcPer == 4, "one 4-, 8- or 16-byte store per thread");
	const uint32_t c0 = (blockIdx.x * kBlock + threadIdx.x) * 4u;
	if (c0 >= n) return;
	const uint32_t has_zero = flags[CC_HAS_ZERO];
	const uint64_t n_unique = static_cast<uint64_t>(flags[CC_COUNT]) + has_zero;
	uint32_t k[4];
#pragma unroll
	for (uint32_t j = 0; j < 4; j++) {
		const uint32_t c = c0 + j;
		k[j] = 0;
		if (c < n && comp_key[c] != zero_key) k[j] = number[root[c]] - (has_zero ? 0u : 1u);
	}
	// the buffer is padded to a multiple of four keys
	if (n_unique <= 0xFFull) *reinterpret_cast<uchar4*>(keys + c0) = make_uchar4(static_cast<unsigned char>(k[0]), static_cast<unsigned char>(k[1]), static_cast<unsigned char>(k[2]), static_cast<unsigned char>(k[3]));
	else if (n_unique <= 0xFFFFull) *reinterpret_cast<ushort4*>(keys + 2ull * c0) = make_ushort4(static_cast<unsigned short>(k[0]), static_cast<unsigned short>(k[1]), static_cast<unsigned short>(k[2]), static_cast<unsigned short>(k[3]));
	else *reinterpret_cast<uint4*>(keys + 4ull * c0) = make_uint4(k[0], k[1], k[2], k[3]);
}

// ------------------------------------------------------------------------------
// dust: components below (or, inverted, at or above) a voxel count lose their label.
//
//   k_cc_voxels    one run per thread (the layout of k_run_links): every foreground run adds its
//                  length to the counter of its component's root.  The runs of a workgroup share few
//                  roots, so the sums are taken in an LDS open-addressing table first (key: the root,
//                  a 32-bit counter: a workgroup's runs lie in one slice and do not intersect, so
//                  their lengths sum to less than 2^32) and flushed with one 64-bit atomic per root.
//                  A root that finds no room in the LDS table adds to its global counter directly:
//                  the global table is indexed by root, it cannot fill.
//   k_edit_mark / k_edit_keys with DustArgs: the label edit (at the end of this file, shared with fill_holes)
// ------------------------------------------------------------------------------
constexpr uint32_t kVoxelLds = 1024;          // LDS table entries (power of two)
constexpr uint32_t kVoxelLdsBits = 10;
constexpr uint32_t kVoxelProbes = 32;         // LDS probes before a run goes to the global counter
static_assert(kVoxelLds == 1u << kVoxelLdsBits, "the hash keeps kVoxelLdsBits bits");

struct VoxelArgs {
	const uint32_t* comp_key;        // [total_comp] label table index of every component (kNoKey: not in the table)
	uint32_t zero_key;               // table index of label 0 (kNoKey: absent): not counted
	uint32_t n_pixels;
	const uint32_t* root;            // [total_comp] k_cc_flatten's roots
	unsigned long long* voxels;      // [total_comp] voxels of the set, at its root; zeroed
	uint32_t* flags;                 // [CC_FLAGS]
};

// grid = (ceil(most runs of a slice / kContactRuns), nslices), block = kContactBlock
static __global__ void __launch_bounds__(kContactBlock) k_cc_voxels(
	RunArrays r, const uint64_t* __restrict__ comp_off, const uint32_t* __restrict__ ncomp_expect, VoxelArgs va
) {
	__shared__ uint32_t s_key[kVoxelLds];
	__shared__ uint32_t s_cnt[kVoxelLds];
	const uint32_t zi = blockIdx.y;
	const uint32_t n = r.nruns[zi];
	const uint32_t i0 = blockIdx.x * kContactRuns;
	if (i0 >= n) return;
	for (uint32_t k = threadIdx.x; k < kVoxelLds; k += kContactBlock) { s_key[k] = kNoKey; s_cnt[k] = 0; }
	__syncthreads();
	const uint64_t rb = r.rbase[zi];
	const uint32_t nce = ncomp_expect[zi];
	const uint32_t off = static_cast<uint32_t>(comp_off[zi]);
	const uint32_t* key_z = va.comp_key + off;
	for (uint32_t k = 0; k < kContactPer; k++) {
		const uint32_t i = i0 + k * kContactBlock + threadIdx.x;
		if (i >= n) break;
		const uint32_t a = r.run_start[rb + i];
		const uint32_t b = i + 1 < n ? r.run_start[rb + i + 1] : va.n_pixels;
		const uint32_t cc = r.run_cc[rb + i];
		const uint32_t ka = cc < nce ? key_z[cc] : kNoKey;
		if (ka == kNoKey) { atomicOr(va.flags + CC_BADKEY, 1u); continue; }
		if (ka == va.zero_key || b <= a) continue;
		const uint32_t root = va.root[off + cc];      // a component id: never kNoKey
		const uint32_t len = b - a;
		const uint32_t h = (root * 0x9E3779B1u) >> (32u - kVoxelLdsBits);
		bool placed = false;
		for (uint32_t p = 0; p < kVoxelProbes && !placed; p++) {
			const uint32_t slot = (h + p) & (kVoxelLds - 1);
			uint32_t cur = s_key[slot];      // a slot changes once, from empty to its key: a stale read is settled by the CAS
			if (cur == kNoKey) {
				cur = atomicCAS(s_key + slot, kNoKey, root);
				if (cur == kNoKey) cur = root;
			}
			if (cur == root) { atomicAdd(s_cnt + slot, len); placed = true; }
		}
		if (!placed) atomicAdd(va.voxels + root, static_cast<unsigned long long>(len));
	}
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < kVoxelLds; k += kContactBlock) {
		const uint32_t root = s_key[k];
		if (root != kNoKey) atomicAdd(va.voxels + root, static_cast<unsigned long long>(s_cnt[k]));
	}
}

// ------------------------------------------------------------------------------
// fill_holes: a background component that touches no face of the volume and whose face neighbours all
// carry one label gets that label.
//
//   k_run_links    in LINK_BACKGROUND mode unites the components of label 0 at the wanted connectivity
//   k_hole_scan    one run per thread (the layout of k_run_links): every run of label 0 looks at its face
//                  neighbours in all six directions and raises the state word of its root
//   k_edit_mark / k_edit_keys with FillArgs: the label edit (below)
//
// The state word of a root, ascending:
//
//   HOLE_NONE (0)  <  1 + k, k a label table index  <  HOLE_MANY  <  HOLE_OPEN
//
// "nothing seen yet", "every face neighbour seen so far has label index k", "two different labels seen",
// "a voxel lies on a face of the volume".  A word only ever rises, and only along NONE -> 1 + k -> MANY
// -> OPEN (steps may be skipped), never from one k to another: NONE becomes 1 + k by compare-and-swap, every
// other step is an atomicMax with MANY or OPEN.  So the final word is a function of the SET of observations,
// not of their order: OPEN if any run lies on a face; else MANY if two runs saw different labels (whichever
// compare-and-swap wins, the loser finds a label that is not its own and raises the word to MANY); else the
// one label seen.  A thread first sums up what its own run sees and issues one update at the end, and none
// where the word read beforehand (relaxed, agent scope, as cc_parent) already says as much: OPEN and MANY are
// final for the walk (a run on a face still raises MANY to OPEN: that test needs no memory), so a run whose
// root is already there does not look at its neighbours at all.  The outside background of a real volume is
// one hole of millions of runs: without the early-out every one of them would send an atomic to one address.
// ------------------------------------------------------------------------------
enum : uint32_t { HOLE_NONE = 0u, HOLE_MANY = 0xFFFFFFFEu, HOLE_OPEN = 0xFFFFFFFFu };      // 1 + k lies between: the host refuses tables of HOLE_MANY - 1 labels or more

struct HoleArgs {
	const uint32_t* comp_key;        // [total_comp] label table index of every component (kNoKey: not in the table)
	uint32_t zero_key;               // table index of label 0 (never kNoKey here: without label 0 the kernel is not launched)
	uint32_t sx, sy, n_pixels, nslices;
	const uint32_t* root;            // [total_comp] k_cc_flatten's roots of the background links
	uint32_t* state;                 // [total_comp] the state word of the set, at its root; zeroed
	uint32_t* flags;                 // [CC_FLAGS]
};

__device__ __forceinline__ uint32_t hole_state(const uint32_t* state, uint32_t root) {
	return __hip_atomic_load(state + root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what a run has seen (HOLE_NONE, 1 + k or HOLE_MANY) and a face neighbour of label index kj (not kNoKey)
__device__ __forceinline__ void hole_see(const HoleArgs& ha, uint32_t& seen, uint32_t kj) {
	if (kj == ha.zero_key) return;      // the same hole, or (connectivity 6) no face neighbour from another one
	if (seen == HOLE_NONE) seen = kj + 1u;
	else if (seen != kj + 1u) seen = HOLE_MANY;
}

// the face neighbours of the run's pixels [x0, x1] in row y of slice zj
__device__ __forceinline__ void hole_row(
	const RunGeom& g, const RunArrays& r, const HoleArgs& ha,
	uint32_t zj, const uint32_t* key_j, uint32_t nce_j, uint32_t y, uint32_t x0, uint32_t x1, uint32_t& seen
) {
	const bool covered = walk_row(g, r, ha.sx, ha.n_pixels, zj, y, x0, x1, [&](uint32_t ccj) {
		const uint32_t kj = ccj < nce_j ? key_j[ccj] : kNoKey;
		if (kj == kNoKey) atomicOr(ha.flags + CC_BADKEY, 1u);
		else hole_see(ha, seen, kj);
	});
	if (!covered) atomicOr(ha.flags + CC_BADKEY, 1u);
}

// grid = (ceil(most runs of a slice / kContactRuns), nslices), block = kContactBlock
static __global__ void __launch_bounds__(kContactBlock) k_hole_scan(
	RunGeom g, RunArrays r, const uint64_t* __restrict__ comp_off, const uint32_t* __restrict__ ncomp_expect, HoleArgs ha
) {
	const uint32_t zi = blockIdx.y;
	const uint32_t n = r.nruns[zi];
	const uint32_t i0 = blockIdx.x * kContactRuns;
	if (i0 >= n) return;
	const uint64_t rb = r.rbase[zi];
	const uint32_t nce = ncomp_expect[zi];
	const uint32_t off = static_cast<uint32_t>(comp_off[zi]);
	const uint32_t* key_z = ha.comp_key + off;
	const bool z_face = zi == 0 || zi + 1 >= ha.nslices;
	// the slices before and after (read for runs that lie on no face only: both exist then)
	const uint32_t zp = zi ? zi - 1 : 0u, zn = zi + 1 < ha.nslices ? zi + 1 : zi;
	const uint32_t nce_p = ncomp_expect[zp], nce_n = ncomp_expect[zn];
	const uint32_t* key_p = ha.comp_key + static_cast<uint32_t>(comp_off[zp]);
	const uint32_t* key_n = ha.comp_key + static_cast<uint32_t>(comp_off[zn]);
	for (uint32_t k = 0; k < kContactPer; k++) {
		const uint32_t i = i0 + k * kContactBlock + threadIdx.x;
		if (i >= n) break;
		const uint32_t a = r.run_start[rb + i];
		const uint32_t b = i + 1 < n ? r.run_start[rb + i + 1] : ha.n_pixels;
		const uint32_t cc = r.run_cc[rb + i];
		const uint32_t ka = cc < nce ? key_z[cc] : kNoKey;
		if (ka == kNoKey) { atomicOr(ha.flags + CC_BADKEY, 1u); continue; }
		if (ka != ha.zero_key || b <= a) continue;
		const uint32_t y = a / ha.sx;
		const uint32_t row = y * ha.sx;
		const uint32_t x0 = a - row, x1 = b - 1 - row;
		const uint32_t root = ha.root[off + cc];      // a component id: below total_comp
		const uint32_t cur = hole_state(ha.state, root);
		if (z_face || x0 == 0 || x1 + 1 >= ha.sx || y == 0 || y + 1 >= ha.sy) {
			if (cur != HOLE_OPEN) atomicMax(ha.state + root, HOLE_OPEN);
			continue;
		}
		if (cur >= HOLE_MANY) continue;      // final: nothing this run sees changes the word
		// the run lies on no face: it is neither first nor last in its row, and rows y - 1, y + 1 and slices zi - 1, zi + 1 exist
		uint32_t seen = HOLE_NONE;
		{
			const uint32_t c0 = r.run_cc[rb + i - 1], c1 = r.run_cc[rb + i + 1];
			const uint32_t k0 = c0 < nce ? key_z[c0] : kNoKey, k1 = c1 < nce ? key_z[c1] : kNoKey;
			if (k0 == kNoKey || k1 == kNoKey) atomicOr(ha.flags + CC_BADKEY, 1u);
			if (k0 != kNoKey) hole_see(ha, seen, k0);
			if (k1 != kNoKey) hole_see(ha, seen, k1);
		}
		hole_row(g, r, ha, zi, key_z, nce, y - 1, x0, x1, seen);
		hole_row(g, r, ha, zi, key_z, nce, y + 1, x0, x1, seen);
		hole_row(g, r, ha, zp, key_p, nce_p, y, x0, x1, seen);
		hole_row(g, r, ha, zn, key_n, nce_n, y, x0, x1, seen);
		if (seen == HOLE_NONE || seen == cur) continue;
		if (seen != HOLE_MANY && cur == HOLE_NONE) {
			const uint32_t old = atomicCAS(ha.state + root, HOLE_NONE, seen);
			if (old == HOLE_NONE || old == seen || old >= HOLE_MANY) continue;
		}
		atomicMax(ha.state + root, HOLE_MANY);      // seen is MANY, or the word holds another label than seen
	}
}

// ------------------------------------------------------------------------------
// The label edit that dust and fill_holes end with: every component gets a new label out of the stream's own
// table (or label 0, whether the table has it or not), decided per component by an Edit:
//
//   e.n, e.comp_key[c], e.root[c]      the components, their label indices and their sets' roots
//   e.new_key(c, key)                  the new label index of component c (label index key, below the table's
//                                      length), or kNoKey for label 0
//   Edit::kGivesZero                   whether new_key ever answers kNoKey (the host then puts 0 into a list without it)
//
//   k_edit_mark    used[new label index] = 1 per component; the roots whose label changes are counted
//   k_edit_keys    every component's key into the new unique list, packed at the key width
//
// The host builds the new list from the `used` bytes in between.
// ------------------------------------------------------------------------------
struct DustArgs {
	const uint32_t* root;                 // [n]
	const uint32_t* comp_key;             // [n]
	const unsigned long long* voxels;     // [n], valid at the roots
	uint32_t zero_key, n;
	unsigned long long threshold;
	uint32_t invert;
	static constexpr bool kGivesZero = true;
	// a component below the threshold (inverted: at or above it) loses its label
	__device__ __forceinline__ uint32_t new_key(uint32_t c, uint32_t key) const {
		return key != zero_key && ((voxels[root[c]] < threshold) != (invert != 0)) ? kNoKey : key;
	}
};

struct FillArgs {
	const uint32_t* root;                 // [n] roots of the background links
	const uint32_t* comp_key;             // [n]
	const uint32_t* state;                // [n] k_hole_scan's words, valid at the roots of label 0's components
	uint32_t zero_key, n;
	static constexpr bool kGivesZero = false;
	// a component of a hole that saw exactly one label takes it
	__device__ __forceinline__ uint32_t new_key(uint32_t c, uint32_t key) const {
		if (key != zero_key) return key;
		const uint32_t s = state[root[c]];
		return s != HOLE_NONE && s < HOLE_MANY ? s - 1u : key;
	}
};

// used[new label index] = 1 for every component; flags[CC_COUNT] += the 3D components whose label changes (their roots)
template <typename Edit>
static __global__ void __launch_bounds__(kBlock) k_edit_mark(Edit e, uint32_t n_table, uint8_t* __restrict__ used, uint32_t* __restrict__ flags) {
	__shared__ uint32_t s_red[kWaves];
	const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
	uint32_t cnt = 0;
	if (c < e.n) {
		const uint32_t key = e.comp_key[c];
		if (key >= n_table) atomicOr(flags + CC_BADKEY, 1u);
		else {
			const uint32_t nk = e.new_key(c, key);
			if (nk < n_table) used[nk] = 1;
			else if (nk != kNoKey) atomicOr(flags + CC_BADKEY, 1u);
			if (nk != key && e.root[c] == c) cnt = 1;
		}
	}
	cnt = block_sum(cnt, s_red);
	if (threadIdx.x == 0 && cnt) atomicAdd(flags + CC_COUNT, cnt);
}

// keys[c] = new_index[new label index of c], or 0 (the place of label 0 in an ascending unsigned list) where c
// gets label 0, at the width of the new list's length: four components per thread, one store
template <typename Edit>
static __global__ void __launch_bounds__(kBlock) k_edit_keys(
	Edit e, uint32_t n_table, const uint32_t* __restrict__ new_index, uint32_t n_unique, uint8_t* __restrict__ keys
) {
	const uint32_t c0 = (blockIdx.x * kBlock + threadIdx.x) * 4u;
	if (c0 >= e.n) return;
	uint32_t k[4];
#pragma unroll
	for (uint32_t j = 0; j < 4; j++) {
		const uint32_t c = c0 + j;
		k[j] = 0;
		if (c < e.n) {
			const uint32_t key = e.comp_key[c];
			const uint32_t nk = key < n_table ? e.new_key(c, key) : kNoKey;
			if (nk < n_table) k[j] = new_index[nk];
		}
	}
	// the buffer is padded to a multiple of four keys
	if (n_unique <= 0xFFu) *reinterpret_cast<uchar4*>(keys + c0) = make_uchar4(static_cast<unsigned char>(k[0]), static_cast<unsigned char>(k[1]), static_cast<unsigned char>(k[2]), static_cast<unsigned char>(k[3]));
	else if (n_unique <= 0xFFFFu) *reinterpret_cast<ushort4*>(keys + 2ull * c0) = make_ushort4(static_cast<unsigned short>(k[0]), static_cast<unsigned short>(k[1]), static_cast<unsigned short>(k[2]), static_cast<unsigned short>(k[3]));
	else *reinterpret_cast<uint4*>(keys + 4ull * c0) = make_uint4(k[0], k[1], k[2], k[3]);
}
