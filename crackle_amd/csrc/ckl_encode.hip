// Encode path: label volume resident in HBM -> .ckl bytes.
// Replaces crackle::compress<LABEL> (src/crackle.hpp:34-257) and what it calls:
//   lib::max_label / pixel_pairs                    src/lib.hpp:224-256        k_stats
//   crackcodes::Graph::init                         src/crackcodes.hpp:66-125  k_label_planes + k_trail_graph (ckl_trail.hpp)
//   create_crack_codes walk + remove_initial_branch +
//     remove_spurious_branches + symbols_to_codepoints
//                                                   src/crackcodes.hpp:128-281, 374-453  k_trail_* (ckl_trail.hpp)
//   pack_codepoints / write_boc_index               src/crackcodes.hpp:318-372, 455-496  k_finish
//   markov::gather_statistics / encode_markov       src/markov.hpp:193-220, 422-473      k_markov_hist / k_markov_pack
//   cc3d::connected_components2d_4 + relabel        src/cc3d.hpp:114-144, 257-369        the flat label stage (ckl_encode_labels.hip)
//   labels::encode_flat                             src/labels.hpp:30-155                the flat label stage (ckl_encode_labels.hip)
//   stream assembly                                 src/crackle.hpp:171-216    host
// The flat label stage and the pin stage (ckl_encode_pins.hip) are units of their own; encode_typed here schedules them
// against the crack trail.  crackle.operations.recompress without the voxels (ckl_recompress.hip) comes in through
// encode_from_planes.
#include "ckl_encoder.hpp"
#include "ckl_encode_labels.hpp"
#include "ckl_decoder.hpp"
#include "ckl_trail.hpp"
#include "ckl_code_words.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <mutex>

namespace ckl {

using namespace dev;

// ------------------------------------------------------------------------------
// whole-volume reductions (lib.hpp:224-256)
// ------------------------------------------------------------------------------
template <typename LABEL>
__global__ void __launch_bounds__(kBlock) k_stats(const LABEL* __restrict__ labels, uint64_t voxels, unsigned long long* __restrict__ out /* [0]=max [1]=pairs */) {
	__shared__ unsigned long long s_max[kWaves], s_pairs[kWaves];
	unsigned long long mx = 0, pairs = 0;
	const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
	for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < voxels; i += stride) {
		const LABEL v = labels[i];
		if (static_cast<unsigned long long>(v) > mx) mx = v;
		if (i > 0) pairs += (labels[i - 1] == v);
	}
	for (int d = kWave / 2; d >= 1; d >>= 1) {
		const unsigned long long om = __shfl_xor(mx, d, kWave);
		const unsigned long long op = __shfl_xor(pairs, d, kWave);
		mx = om > mx ? om : mx;
		pairs += op;
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (lane == 0) { s_max[wave] = mx; s_pairs[wave] = pairs; }
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < kWaves; w++) { mx = s_max[w] > mx ? s_max[w] : mx; pairs += s_pairs[w]; }
		atomicMax(out, mx);
		atomicAdd(out + 1, pairs);
	}
}

// ------------------------------------------------------------------------------
// label planes: one pass over the labels produces, per slice, two row-aligned bit
// planes of "differs from the left neighbour" (V) and "differs from the upper
// neighbour" (H).  Both the crack graph (crackcodes.hpp:66-125) and the 4-connected
// components (cc3d.hpp:257-369) are derived from these 0.25 B/voxel instead of
// re-reading the labels.  One wavefront per 64 pixels of a row: coalesced loads, the
// left neighbour comes from a lane shuffle, the plane words from a ballot.
// grid = (ceil(chunks_per_row * sy / 4), nslices), chunks_per_row = ceil(sx / 64)
// ------------------------------------------------------------------------------
constexpr uint32_t kPlaneUnroll = 4;   // 64-pixel chunks per wavefront (loads issued together)

template <typename LABEL>
__global__ void __launch_bounds__(kBlock) k_label_planes(
	const LABEL* __restrict__ labels, uint32_t sx, uint32_t sy, uint32_t chunks_per_row,
	uint32_t* __restrict__ planeV, uint32_t* __restrict__ planeH, uint32_t row_words, uint64_t plane_words,
	uint32_t* __restrict__ count_v, uint32_t* __restrict__ count_h
) {
	__shared__ uint32_t s_red[2 * kWaves];
	const uint32_t zi = blockIdx.y;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t units = chunks_per_row * sy;
	const uint32_t unit0 = (blockIdx.x * kWaves + wave) * kPlaneUnroll;
	const LABEL* slice = labels + static_cast<uint64_t>(zi) * sy * sx;
	LABEL v[kPlaneUnroll], up[kPlaneUnroll], lf[kPlaneUnroll];
	uint32_t xs[kPlaneUnroll], ys[kPlaneUnroll];
#pragma unroll
	for (uint32_t k = 0; k < kPlaneUnroll; k++) {
		const uint32_t unit = unit0 + k;
		const uint32_t y = unit / chunks_per_row;
		const uint32_t x = (unit - y * chunks_per_row) * 64u + lane;
		xs[k] = x; ys[k] = y;
		const bool valid = unit < units && x < sx;
		const LABEL* row = slice + static_cast<uint64_t>(y) * sx;
		v[k] = valid ? row[x] : LABEL(0);
		up[k] = (valid && y > 0) ? row[static_cast<int64_t>(x) - static_cast<int64_t>(sx)] : v[k];
		lf[k] = (valid && lane == 0 && x > 0) ? row[x - 1] : v[k];
	}
	uint32_t nv = 0, nh = 0;
#pragma unroll
	for (uint32_t k = 0; k < kPlaneUnroll; k++) {
		const uint32_t unit = unit0 + k;
		const bool valid = unit < units && xs[k] < sx;
		LABEL left = __shfl_up(v[k], 1, kWave);
		if (lane == 0) left = lf[k];
		const bool dv = valid && xs[k] > 0 && v[k] != left;
		const bool dh = valid && v[k] != up[k];
		const unsigned long long mv = __ballot(dv), mh = __ballot(dh);
		if (lane == 0 && unit < units) {
			const uint32_t c = xs[k] >> 6;
			const uint64_t wbase = zi * plane_words + static_cast<uint64_t>(ys[k]) * row_words + c * 2u;
			planeV[wbase] = static_cast<uint32_t>(mv);
			planeH[wbase] = static_cast<uint32_t>(mh);
			if (c * 2u + 1u < row_words) {
				planeV[wbase + 1] = static_cast<uint32_t>(mv >> 32);
				planeH[wbase + 1] = static_cast<uint32_t>(mh >> 32);
			}
			nv += __popcll(mv);
			nh += __popcll(mh);
		}
	}
	if (lane == 0) { s_red[wave] = nv; s_red[kWaves + wave] = nh; }
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t tv = 0, th = 0;
		for (int w = 0; w < kWaves; w++) { tv += s_red[w]; th += s_red[kWaves + w]; }
		if (tv) atomicAdd(count_v + zi, tv);
		if (th) atomicAdd(count_h + zi, th);
	}
}

// Fast path (sx a multiple of the 16-byte vector, 16-byte aligned volume): one wavefront
// owns a strip of 64 vectors x kBandRows rows and walks down it, so every label is loaded
// once with 16-byte loads (the row above stays in registers) and the same pass yields
// lib::max_label and lib::pixel_pairs (lib.hpp:224-256).  Plane words are assembled from
// the per-lane bit groups with an OR butterfly.  No atomics: per-workgroup partial counts
// go to `partial` and are folded per slice by k_planes_reduce.
// grid = (ceil(strips * bands / 4), nslices)
constexpr uint32_t kBandRows = 32;

// 16 bytes that nobody reads again
template <typename V, typename T>
__device__ __forceinline__ V nt_load_vec(const T* p) {
	typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
	static_assert(sizeof(V) == 16, "one 16-byte vector");
	const u32x4_t raw = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
	V v;
	__builtin_memcpy(&v, &raw, 16);
	return v;
}

// The label-planes pass with nothing but label loads in the wavefront's memory queue (round 5).  Round 1's kernel
// (since removed) stored two plane words per row from inside its row loop; loads and stores retire on ONE counter on
// this architecture and "mixed" means "wait for all": every group of four rows drained its stores before the next
// loads went out, and that kernel read 2.15 GB in 0.42 - 0.46 ms where a plain read takes 0.31.  Here a row's plane words go to LDS (2 KiB per
// wavefront for a strip of 32 rows) and leave in two 16-byte stores per lane after the loop; the label of the pixel left
// of the strip is a SCALAR load (its own counter); and the rows sit in a window of kRowsAhead registers that is
// refilled as it is consumed, so that kRowsAhead - 1 row loads are always in flight.
// (or_over_lane_group / wave_shift_up1_label: DPP instead of ds_bpermute.)  Same grid, same outputs.
template <typename T>
__device__ __forceinline__ T wave_shift_up1_label(T v) {
	if constexpr (sizeof(T) == 8) {
		const uint32_t lo = dev::wave_shift_up1(static_cast<uint32_t>(v), 0u), hi = dev::wave_shift_up1(static_cast<uint32_t>(static_cast<uint64_t>(v) >> 32), 0u);
		return static_cast<T>((static_cast<uint64_t>(hi) << 32) | lo);
	}
	else return static_cast<T>(dev::wave_shift_up1(static_cast<uint32_t>(v), 0u));
}
// OR of a value over every aligned group of G lanes (2, 4, 8, 16), the result in all lanes of the group: quad permutes,
// then mirrors of half a row / a row of 16 lanes (a mirror pairs every lane with one of the other half: all an OR needs)
template <uint32_t G>
__device__ __forceinline__ uint32_t or_over_lane_group(uint32_t v) {
	static_assert(G == 2 || G == 4 || G == 8 || G == 16, "lane groups inside a row of 16");
	if constexpr (G >= 2) v |= dev::dpp_u32<0xB1, 0xF>(0u, v);      // quad_perm [1, 0, 3, 2]
	if constexpr (G >= 4) v |= dev::dpp_u32<0x4E, 0xF>(0u, v);      // quad_perm [2, 3, 0, 1]
	if constexpr (G >= 8) v |= dev::dpp_u32<0x141, 0xF>(0u, v);     // row_half_mirror
	if constexpr (G >= 16) v |= dev::dpp_u32<0x140, 0xF>(0u, v);    // row_mirror
	return v;
}

template <typename LABEL>
__global__ void __launch_bounds__(kBlock) k_label_planes_stream(
	const LABEL* __restrict__ labels, uint32_t sx, uint32_t sy, uint32_t strips, uint32_t bands,
	uint32_t* __restrict__ planeV, uint32_t* __restrict__ planeH, uint32_t row_words, uint64_t plane_words,
	uint32_t* __restrict__ partial, unsigned long long* __restrict__ partial_max, unsigned long long* __restrict__ total_pairs
) {
	if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *total_pairs = 0;
	constexpr uint32_t P = 16 / sizeof(LABEL);        // pixels per lane
	constexpr uint32_t G = 32 / P;                    // lanes per plane word
	constexpr uint32_t WPR = 64 / G;                  // plane words of a strip's row
	struct alignas(16) Vec { LABEL v[P]; };
	__shared__ uint32_t s_red[3 * kWaves];
	__shared__ unsigned long long s_max[kWaves];
	__shared__ __attribute__((aligned(16))) uint32_t s_words[kWaves][2][kBandRows * WPR];      // plane words of the wavefront's strip: V, H
	const uint32_t zi = blockIdx.y;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t task = blockIdx.x * kWaves + wave;
	uint32_t nv = 0, nh = 0, pairs = 0;
	LABEL mxl = 0;
	if (task < strips * bands) {
		const uint32_t band = __builtin_amdgcn_readfirstlane(task / strips), strip = __builtin_amdgcn_readfirstlane(task - (task / strips) * strips);
		const uint32_t x0 = strip * (64u * P);            // the strip's first pixel column (wave-uniform)
		const uint32_t x = x0 + lane * P;
		const uint32_t y0 = band * kBandRows, y1 = min(y0 + kBandRows, sy);
		const bool active = x < sx;
		const uint64_t slice_off = static_cast<uint64_t>(zi) * sy * sx;
		const LABEL* col = labels + slice_off + (active ? x : 0u);      // (lanes past the row's end load the row's first vector: every load is unconditional)
		Vec prev;
#pragma unroll
		for (uint32_t i = 0; i < P; i++) prev.v[i] = 0;
		if (y0 > 0) prev = nt_load_vec<Vec>(col + static_cast<uint64_t>(y0 - 1) * sx);
		uint32_t* sv = s_words[wave][0];
		uint32_t* sh = s_words[wave][1];
		// the pixel before the strip's first one in LINEAR order (the previous row / slice when the strip starts a row):
		// one label per row, the same for the whole wavefront -> a scalar load of the 4 bytes that hold it
		auto edge_of = [&](uint32_t y, bool& have) -> LABEL {
			const uint64_t lin = slice_off + static_cast<uint64_t>(y) * sx + x0;      // wave-uniform
			have = lin > 0;
			const uint64_t at = have ? lin - 1 : 0;
			if constexpr (sizeof(LABEL) >= 4) return labels[at];
			else {
				const uint64_t byte = at * sizeof(LABEL);
				const uint32_t w = reinterpret_cast<const uint32_t*>(reinterpret_cast<uintptr_t>(labels) & ~static_cast<uintptr_t>(3))[(byte + (reinterpret_cast<uintptr_t>(labels) & 3u)) >> 2];
				return static_cast<LABEL>(w >> (8u * static_cast<uint32_t>((byte + (reinterpret_cast<uintptr_t>(labels) & 3u)) & 3u)));
			}
		};
		constexpr uint32_t kRowsAhead = 4;
		Vec rows[kRowsAhead];
		LABEL edges[kRowsAhead];
		bool have_edges[kRowsAhead];
		auto request = [&](uint32_t r, uint32_t y) {
			const uint32_t yl = y < y1 ? y : y1 - 1u;      // (rows past the band re-read its last row: no load in a branch of its own)
			rows[r] = nt_load_vec<Vec>(col + static_cast<uint64_t>(yl) * sx);
			edges[r] = edge_of(yl, have_edges[r]);
		};
#pragma unroll
		for (uint32_t r = 0; r < kRowsAhead; r++) request(r, y0 + r);
		// (a fixed trip count, fully unrolled: straight-line code, so that the compiler waits for exactly the load a row
		// needs — across a loop's back edge it waits for all of them)
#pragma unroll
		for (uint32_t it = 0; it < kBandRows / kRowsAhead; it++) {
			const uint32_t yb = y0 + it * kRowsAhead;
#pragma unroll
			for (uint32_t r = 0; r < kRowsAhead; r++) {
				const uint32_t y = yb + r;
				const Vec cur = rows[r];
				const LABEL edge = edges[r];
				const bool have_edge = have_edges[r];
				request(r, y + kRowsAhead);      // the slot is free: its next row goes out before this one is looked at
				if (y >= y1) continue;
				LABEL left = wave_shift_up1_label(cur.v[P - 1]);
				bool have_left = true;
				if (lane == 0) { left = edge; have_left = have_edge; }
				uint32_t bv = 0, bh = 0;
				if (active) {
#pragma unroll
					for (uint32_t i = 0; i < P; i++) {
						const LABEL l = i ? cur.v[i - 1] : left;
						bv |= (cur.v[i] != l ? 1u : 0u) << i;
						bh |= (cur.v[i] != prev.v[i] ? 1u : 0u) << i;
						mxl = cur.v[i] > mxl ? cur.v[i] : mxl;
					}
					// lib::pixel_pairs counts equal LINEAR neighbours (lib.hpp:249-256): every pixel but the volume's first has one
					pairs += P - __popc(bv) - ((have_left || (bv & 1u)) ? 0u : 1u);
					if (x == 0) bv &= ~1u;      // no crack along the image's left border
					if (y == 0) bh = 0u;
				}
				nv += __popc(bv); nh += __popc(bh);
				bv <<= (lane % G) * P; bh <<= (lane % G) * P;
				bv = or_over_lane_group<G>(bv); bh = or_over_lane_group<G>(bh);
				if ((lane % G) == 0) { sv[(y - y0) * WPR + lane / G] = bv; sh[(y - y0) * WPR + lane / G] = bh; }
				prev = cur;
			}
		}
		// the strip's plane words out: row r of the band, words word0 .. word0 + WPR - 1 of the row (LDS accesses of one
		// wavefront are ordered: no barrier)
		const uint32_t word0 = x0 >> 5;
		uint32_t* pv = planeV + zi * plane_words;
		uint32_t* ph = planeH + zi * plane_words;
		constexpr uint32_t kVecWords = WPR >= 4 ? 4u : WPR;      // words per lane and store
		constexpr uint32_t kLanesPerRow = WPR / kVecWords;
		for (uint32_t r0 = 0; r0 < y1 - y0; r0 += 64u / kLanesPerRow) {
			const uint32_t r = r0 + lane / kLanesPerRow, w = (lane % kLanesPerRow) * kVecWords;
			if (r >= y1 - y0) continue;
			const uint64_t at = static_cast<uint64_t>(y0 + r) * row_words + word0 + w;
			if (word0 + w + kVecWords <= row_words && ((at & (kVecWords - 1u)) == 0u) && kVecWords == 4u) {
				*reinterpret_cast<uint4*>(pv + at) = *reinterpret_cast<const uint4*>(sv + r * WPR + w);
				*reinterpret_cast<uint4*>(ph + at) = *reinterpret_cast<const uint4*>(sh + r * WPR + w);
			}
			else {
				for (uint32_t q = 0; q < kVecWords; q++) if (word0 + w + q < row_words) { pv[at + q] = sv[r * WPR + w + q]; ph[at + q] = sh[r * WPR + w + q]; }
			}
		}
	}
	nv = wave_sum(nv); nh = wave_sum(nh); pairs = wave_sum(pairs);
	unsigned long long mx = static_cast<unsigned long long>(mxl);
	for (int d = kWave / 2; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(mx, d, kWave); mx = o > mx ? o : mx; }
	if (lane == 0) { s_red[wave] = nv; s_red[kWaves + wave] = nh; s_red[2 * kWaves + wave] = pairs; s_max[wave] = mx; }
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t tv = 0, th = 0, tp = 0;
		unsigned long long tm = 0;
		for (int w = 0; w < kWaves; w++) { tv += s_red[w]; th += s_red[kWaves + w]; tp += s_red[2 * kWaves + w]; tm = s_max[w] > tm ? s_max[w] : tm; }
		const uint64_t o = static_cast<uint64_t>(zi) * gridDim.x + blockIdx.x;
		partial[o * 4 + 0] = tv; partial[o * 4 + 1] = th; partial[o * 4 + 2] = tp; partial[o * 4 + 3] = 0;
		partial_max[o] = tm;
	}
}

// ckl_reencode_markov: the decoder's crack planes become the encoder's "differs from the
// neighbour" planes (a crack is a differing pair for IMPERMISSIBLE streams and an equal pair for
// PERMISSIBLE ones; image-border pairs carry neither) with their per-slice population counts.
// grid = (ceil(plane_words / 256), nslices); counts: [nslices] v, then [nslices] h, zeroed by the host
__global__ void __launch_bounds__(kBlock) k_planes_from_cracks(
	const uint32_t* __restrict__ crackV, const uint32_t* __restrict__ crackH, uint32_t sx, uint32_t sy,
	uint32_t row_words, uint64_t plane_words, uint32_t permissible,
	uint32_t* __restrict__ planeV, uint32_t* __restrict__ planeH, uint32_t* __restrict__ counts, uint32_t nslices
) {
	__shared__ uint32_t s_red[kWaves];
	const uint32_t zi = blockIdx.y;
	const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
	uint32_t nv = 0, nh = 0;
	if (i < plane_words) {
		const uint32_t y = static_cast<uint32_t>(i / row_words);
		const uint32_t w = static_cast<uint32_t>(i - static_cast<uint64_t>(y) * row_words);
		const uint32_t left = sx - w * 32u;
		const uint32_t in_row = left >= 32u ? 0xFFFFFFFFu : ((1u << left) - 1u);           // x < sx
		const uint32_t mv = in_row & (w == 0 ? 0xFFFFFFFEu : 0xFFFFFFFFu);                   // 1 <= x < sx
		const uint32_t mh = y >= 1 ? in_row : 0u;                                            // y >= 1
		const uint64_t at = zi * plane_words + i;
		const uint32_t inv = permissible ? 0xFFFFFFFFu : 0u;
		const uint32_t v = (crackV[at] ^ inv) & mv, h = (crackH[at] ^ inv) & mh;
		planeV[at] = v; planeH[at] = h;
		nv = __popc(v); nh = __popc(h);
	}
	nv = block_sum(nv, s_red); nh = block_sum(nh, s_red);
	if (threadIdx.x == 0) {
		if (nv) atomicAdd(counts + zi, nv);
		if (nh) atomicAdd(counts + nslices + zi, nh);
	}
}

// grid = nslices: folds the per-workgroup partials of one slice
__global__ void __launch_bounds__(kBlock) k_planes_reduce(
	const uint32_t* __restrict__ partial, const unsigned long long* __restrict__ partial_max, uint32_t nblk,
	unsigned long long* __restrict__ out /* [nslices][4]: count_v, count_h, pairs, max */,
	unsigned long long* __restrict__ total_pairs /* the volume's equal pixel pairs: k_trail_graph decides the crack format from it */
) {
	__shared__ uint32_t s_red[kWaves];
	__shared__ unsigned long long s_max[kWaves];
	const uint32_t zi = blockIdx.x;
	uint32_t tv = 0, th = 0, tp = 0;
	unsigned long long tm = 0;
	for (uint32_t b = threadIdx.x; b < nblk; b += kBlock) {
		const uint64_t o = static_cast<uint64_t>(zi) * nblk + b;
		tv += partial[o * 4 + 0]; th += partial[o * 4 + 1]; tp += partial[o * 4 + 2];
		const unsigned long long m = partial_max[o];
		tm = m > tm ? m : tm;
	}
	tv = block_sum(tv, s_red); th = block_sum(th, s_red); tp = block_sum(tp, s_red);
	for (int d = kWave / 2; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(tm, d, kWave); tm = o > tm ? o : tm; }
	if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = tm;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 0; w < kWaves; w++) tm = s_max[w] > tm ? s_max[w] : tm;
		out[4ull * zi + 0] = tv; out[4ull * zi + 1] = th; out[4ull * zi + 2] = tp; out[4ull * zi + 3] = tm;
		atomicAdd(total_pairs, static_cast<unsigned long long>(tp));
	}
}

enum : uint8_t { CODE_UP = 0, CODE_RIGHT = 1, CODE_DOWN = 2, CODE_LEFT = 3, CODE_NONE = 0xFE, CODE_TOMB = 0xFF };

// ------------------------------------------------------------------------------
// k_finish: chain order, compaction, difference coding, 2-bit packing, BOC index
// (crackcodes.hpp:318-372, 455-496); one workgroup per slice.
// ------------------------------------------------------------------------------
struct FinishArgs {
	int sx, sy, xw, yw;
	uint32_t z0;               // first slice of this launch
	uint32_t markov;           // 1: write difference codes to dcode instead of packing
	const uint64_t* cbase;
	const uint64_t* kbase;
	const uint32_t* n_chains;
	const uint32_t* n_raw;
	const uint32_t* n_valid;
	const uint8_t* cp;
	const uint32_t* chain_node;
	const uint32_t* chain_off;
	const uint32_t* chain_clen;
	uint32_t* chain_order;     // scratch [kcap]
	uint32_t* chain_dst;       // scratch [kcap]
	uint32_t* chain_vstart;    // scratch [kcap]
	uint8_t* fcode;            // final-order code points   (at cbase)
	uint8_t* dcode;            // final-order difference codes (at cbase; markov only)
	const uint64_t* pbase;     // per slice: base into payload (4-byte aligned)
	uint8_t* payload;
	const uint64_t* bbase;     // per slice: base into boc
	uint8_t* boc;
	uint32_t* payload_len;     // [nslices]
	uint32_t* boc_len;         // [nslices]
};

__device__ __forceinline__ void put_le_dev(uint8_t* p, uint32_t v, int w) {
	for (int i = 0; i < w; i++) p[i] = static_cast<uint8_t>((v >> (8 * i)) & 0xFF);
}

// 1024 threads per slice: two workgroups share a CU, and the phases below are rounds of
// latency-bound byte accesses, so the time goes with the rounds per thread
constexpr int kFinishBlock = 1024;
constexpr int kFinishWaves = kFinishBlock / kWave;

// chains of a slice whose tables k_finish stages in LDS (a slice of the bench volume has ~100; noise has thousands)
constexpr uint32_t kFinishChains = 2048;

__global__ void __launch_bounds__(kFinishBlock) k_finish(FinishArgs a) {
	__shared__ uint32_t s_scan[kFinishWaves];
	// phase 1 is one thread's serial walk over the chains — an insertion sort and the BOC index, every step a
	// dependent access — and in global memory each of those was a trip of a microsecond: a third of the kernel.  The
	// chain tables are staged here (5 x 8 KiB; two workgroups share a CU) and phase 2 reads them back from here.
	__shared__ uint32_t s_node[kFinishChains], s_clen[kFinishChains], s_off[kFinishChains], s_ord[kFinishChains], s_dst[kFinishChains], s_vst[kFinishChains];
	const uint32_t zi = blockIdx.x + a.z0;
	const int tid = threadIdx.x;
	const uint32_t nch = a.n_chains[zi], nraw = a.n_raw[zi], nvalid = a.n_valid[zi];
	const uint8_t* cp = a.cp + a.cbase[zi];
	uint8_t* fcode = a.fcode + a.cbase[zi];
	const bool staged = nch <= kFinishChains;      // uniform
	const uint32_t* ch_node = a.chain_node + a.kbase[zi];
	const uint32_t* ch_off = a.chain_off + a.kbase[zi];
	const uint32_t* ch_clen = a.chain_clen + a.kbase[zi];
	uint32_t* order = a.chain_order + a.kbase[zi];
	uint32_t* dst = a.chain_dst + a.kbase[zi];
	uint32_t* vstart = a.chain_vstart + a.kbase[zi];
	if (staged) {
		for (uint32_t c = tid; c < nch; c += kFinishBlock) { s_node[c] = ch_node[c]; s_clen[c] = ch_clen[c]; s_off[c] = ch_off[c]; }
		__syncthreads();
		ch_node = s_node; ch_off = s_off; ch_clen = s_clen; order = s_ord; dst = s_dst; vstart = s_vst;
	}
	const uint32_t sxe = a.sx + 1;

	// ---- phase 1 (serial over chains): order by start vertex, output offsets, BOC index ----
	if (tid == 0) {
		uint32_t v = 0;
		for (uint32_t c = 0; c < nch; c++) { vstart[c] = v; v += ch_clen[c]; }
		// chains come out in ascending raw start order and remove_initial_branch only
		// moves a start inside its own component: insertion sort on a nearly sorted list
		for (uint32_t c = 0; c < nch; c++) {
			const uint32_t key = ch_node[c];
			uint32_t p = c;
			while (p > 0 && ch_node[order[p - 1]] > key) { order[p] = order[p - 1]; p--; }
			order[p] = c;
		}
		uint32_t d = 0;
		for (uint32_t i = 0; i < nch; i++) { dst[order[i]] = d; d += ch_clen[order[i]]; }

		// write_boc_index (crackcodes.hpp:318-372)
		uint8_t* b = a.boc + a.bbase[zi];
		uint32_t num_y = 0, index_size = a.yw;
		for (uint32_t i = 0; i < nch;) {
			const uint32_t y = ch_node[order[i]] / sxe;
			uint32_t j = i;
			while (j < nch && ch_node[order[j]] / sxe == y) j++;
			index_size += a.yw + (j - i + 1) * a.xw;
			num_y++;
			i = j;
		}
		uint32_t idx = 0;
		put_le_dev(b + idx, index_size, 4); idx += 4;
		put_le_dev(b + idx, num_y, a.yw); idx += a.yw;
		uint32_t last_y = 0;
		for (uint32_t i = 0; i < nch;) {
			const uint32_t y = ch_node[order[i]] / sxe;
			uint32_t j = i;
			while (j < nch && ch_node[order[j]] / sxe == y) j++;
			put_le_dev(b + idx, y - last_y, a.yw); idx += a.yw;
			last_y = y;
			put_le_dev(b + idx, j - i, a.xw); idx += a.xw;
			uint32_t last_x = 0;
			for (uint32_t k = i; k < j; k++) {
				const uint32_t x = ch_node[order[k]] - sxe * y;
				put_le_dev(b + idx, x - last_x, a.xw); idx += a.xw;
				last_x = x;
			}
			i = j;
		}
		a.boc_len[zi] = idx;
	}
	__syncthreads();
	__threadfence_block();

	// ---- phase 2: scatter of each chain to its sorted place.  A permutation of chains: no kernel writes CODE_TOMB any
	// more (k_trail_items lets the vanishing 'b' / 't' pairs vanish before a code exists, n_valid = n_raw), the
	// compaction below finds nothing to compact ----
	constexpr uint32_t kPer = 16;
	uint32_t carry = 0;
	for (uint32_t tile = 0; tile < nraw; tile += kFinishBlock * kPer) {
		const uint32_t i0 = tile + tid * kPer;
		uint32_t cnt = 0;
		uint8_t c[kPer];
		static_assert(kPer == 16, "one 16-byte load per thread");
		if (i0 + kPer <= nraw) {      // (the slice's codes start 16-byte aligned: crack_pass rounds the capacities)
			const uint4 v = *reinterpret_cast<const uint4*>(cp + i0);
			const uint32_t w4[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
			for (uint32_t k = 0; k < kPer; k++) c[k] = static_cast<uint8_t>(w4[k >> 2] >> (8u * (k & 3u)));
		}
		else {
#pragma unroll
			for (uint32_t k = 0; k < kPer; k++) { const uint32_t i = i0 + k; c[k] = i < nraw ? cp[i] : CODE_TOMB; }
		}
#pragma unroll
		for (uint32_t k = 0; k < kPer; k++) cnt += (c[k] != CODE_TOMB);
		uint32_t v[1] = { cnt }, tot[1];
		block_excl_add<1, kFinishWaves>(v, tot, s_scan);
		uint32_t g = carry + v[0];
		if (cnt) {
			// chain of raw index i0: last chain with ch_off <= i0
			uint32_t lo = 0, hi = nch;
			while (lo + 1 < hi) {
				const uint32_t mid = (lo + hi) >> 1;
				if (ch_off[mid] <= i0) lo = mid; else hi = mid;
			}
			uint32_t chain = lo;
			uint32_t next_off = (chain + 1 < nch) ? ch_off[chain + 1] : 0xFFFFFFFFu;
			if (i0 + kPer <= next_off) {
				// all sixteen in one chain (a slice has ~100 chains in 128 k codes): the surviving codes go out together — one
				// unaligned 16-byte store when none is a tombstone, else 8 + 4 + 2 + 1 — instead of a store per byte (67 M one-byte
				// requests at C2 ran at the L2s' request rate)
				struct __attribute__((packed)) U128 { uint4 v; };
				struct __attribute__((packed)) U64 { unsigned long long v; };
				struct __attribute__((packed)) U32 { uint32_t v; };
				struct __attribute__((packed)) U16 { uint16_t v; };
				uint8_t* d = fcode + dst[chain] + (g - vstart[chain]);
				unsigned long long w0 = 0, w1 = 0;
				uint32_t m = 0;
#pragma unroll
				for (uint32_t k = 0; k < kPer; k++) {
					if (c[k] != CODE_TOMB) {
						if (m < 8u) w0 |= static_cast<unsigned long long>(c[k]) << (8u * m);
						else w1 |= static_cast<unsigned long long>(c[k]) << (8u * (m - 8u));
						m++;
					}
				}
				if (m == 16u) reinterpret_cast<U128*>(d)->v = make_uint4(static_cast<uint32_t>(w0), static_cast<uint32_t>(w0 >> 32), static_cast<uint32_t>(w1), static_cast<uint32_t>(w1 >> 32));
				else {
					if (m & 8u) { reinterpret_cast<U64*>(d)->v = w0; d += 8; w0 = w1; }
					if (m & 4u) { reinterpret_cast<U32*>(d)->v = static_cast<uint32_t>(w0); d += 4; w0 >>= 32; }
					if (m & 2u) { reinterpret_cast<U16*>(d)->v = static_cast<uint16_t>(w0); d += 2; w0 >>= 16; }
					if (m & 1u) d[0] = static_cast<uint8_t>(w0);
				}
			}
			else {
#pragma unroll
				for (uint32_t k = 0; k < kPer; k++) {
					const uint32_t i = i0 + k;
					while (i >= next_off) { chain++; next_off = (chain + 1 < nch) ? ch_off[chain + 1] : 0xFFFFFFFFu; }
					if (c[k] != CODE_TOMB) {
						fcode[dst[chain] + (g - vstart[chain])] = c[k];
						g++;
					}
				}
			}
		}
		carry += tot[0];
	}
	__syncthreads();
	__threadfence_block();

	// ---- phase 3: whole-slice mod-4 difference code, then 2-bit packing ----
	if (a.markov) {
		uint8_t* dcode = a.dcode + a.cbase[zi];
		for (uint32_t g = tid; g < nvalid; g += kFinishBlock) {
			const uint32_t prev = g ? fcode[g - 1] : 0u;
			dcode[g] = static_cast<uint8_t>((fcode[g] - prev) & 3u);
		}
		if (tid == 0) a.payload_len[zi] = 0;
	}
	else {
		uint8_t* out = a.payload + a.pbase[zi];        // 4-byte aligned
		const uint32_t nbytes = (nvalid + 3) / 4;
		const uint32_t nwords = (nvalid + 15) / 16;
		// 16 codes -> one 32-bit word per thread and step (one 16-byte load, one 4-byte store)
		for (uint32_t w = tid; w < nwords; w += kFinishBlock) {
			const uint32_t g0 = w * 16u;
			uint8_t c[16];
			if (g0 + 16u <= nvalid) {
				const uint4 v = *reinterpret_cast<const uint4*>(fcode + g0);
				const uint32_t w4[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
				for (uint32_t j = 0; j < 16; j++) c[j] = static_cast<uint8_t>(w4[j >> 2] >> (8u * (j & 3u)));
			}
			else {
#pragma unroll
				for (uint32_t j = 0; j < 16; j++) c[j] = g0 + j < nvalid ? fcode[g0 + j] : 0;
			}
			uint32_t prev = g0 ? fcode[g0 - 1] : 0u;
			uint32_t enc = 0;
#pragma unroll
			for (uint32_t j = 0; j < 16; j++) {
				if (g0 + j < nvalid) enc |= ((c[j] - prev) & 3u) << (2 * j);
				prev = c[j];
			}
			if (4u * w + 4u <= nbytes) reinterpret_cast<uint32_t*>(out)[w] = enc;
			else for (uint32_t k = 4u * w; k < nbytes; k++) out[k] = static_cast<uint8_t>(enc >> (8u * (k - 4u * w)));
		}
		if (tid == 0) a.payload_len[zi] = nbytes;
	}
}

// ------------------------------------------------------------------------------
// k_trail_emit: k_trail_offsets + k_trail_expand + k_finish in one workgroup per slice, the code points packed in LDS.
// The three kernels move every code point through HBM three times as a byte (expanded, permuted, read for the
// difference) although it exists packed beside its dart and every chain's final place is known before the first code
// point is expanded.  Here an item ORs its code points, 2 bits each, into a buffer of words in LDS at their FINAL
// index; the difference code is taken on the words (ckl_code_words.hpp) and the words are stored.  No workgroup waits
// for another.
//
// Dynamic LDS, in words: item0[tcap] | dst[tcap] | words[wcap], where the chain tables that only the chain phase
// reads (node, order, vstart: 3 tcap words) lie over the beginning of words[] until the words are zeroed.  A slice with
// more than tcap chains keeps its chain tables in global memory (as k_finish does above kFinishChains); a slice with
// more than 16 wcap code points — the host sizes wcap from an estimate, emit_plan — is emitted in windows of wcap
// words, every item looking at every window.
// ------------------------------------------------------------------------------
constexpr int kEmitBlock = 1024;
constexpr int kEmitWaves = kEmitBlock / kWave;
constexpr uint32_t kEmitLong = 1024;      // segments to walk that the workgroup lists; a slice with more has them walked by the threads that meet them

// what k_trail_emit does behind the offsets, on chain tables in LDS (a slice of up to tcap chains) or in global memory: the
// caller hands the tables over so that each instance addresses its own memory (a pointer that may be either costs a flat
// access, which waits for the loads in flight as well)
struct EmitSlice {
	uint32_t zi, n, nch, total, wcap;
	const uint32_t* items;
	const uint32_t* off;
	const uint32_t* dlen;
	uint64_t nb;
};

__device__ __forceinline__ void emit_chains_and_codes(
	const TrailArgs& a, const FinishArgs& f, const EmitSlice& sl, uint32_t* words,
	const uint32_t* ch_node, const uint32_t* item0, const uint32_t* vstart, uint32_t* order, uint32_t* dst,
	const uint32_t* s_long, const uint32_t* s_nlong, uint32_t* s_carry
) {
	const uint32_t tid = threadIdx.x;
	const uint32_t zi = sl.zi, n = sl.n, nch = sl.nch, total = sl.total;
	const uint32_t sxe = f.sx + 1;

	// ---- chains (k_finish phase 1, serial over chains): order by start vertex, output offsets, BOC index ----
	if (tid == 0) {
		auto clen = [&](uint32_t c) -> uint32_t { return (c + 1 < nch ? vstart[c + 1] : total) - vstart[c]; };
		// chains come out in ascending raw start order and remove_initial_branch only
		// moves a start inside its own component: insertion sort on a nearly sorted list
		for (uint32_t c = 0; c < nch; c++) {
			const uint32_t key = ch_node[c];
			uint32_t p = c;
			while (p > 0 && ch_node[order[p - 1]] > key) { order[p] = order[p - 1]; p--; }
			order[p] = c;
		}
		uint32_t d = 0;
		for (uint32_t i = 0; i < nch; i++) { dst[order[i]] = d; d += clen(order[i]); }

		// write_boc_index (crackcodes.hpp:318-372)
		uint8_t* b = f.boc + f.bbase[zi];
		uint32_t num_y = 0, index_size = f.yw;
		for (uint32_t i = 0; i < nch;) {
			const uint32_t y = ch_node[order[i]] / sxe;
			uint32_t j = i;
			while (j < nch && ch_node[order[j]] / sxe == y) j++;
			index_size += f.yw + (j - i + 1) * f.xw;
			num_y++;
			i = j;
		}
		uint32_t idx = 0;
		put_le_dev(b + idx, index_size, 4); idx += 4;
		put_le_dev(b + idx, num_y, f.yw); idx += f.yw;
		uint32_t last_y = 0;
		for (uint32_t i = 0; i < nch;) {
			const uint32_t y = ch_node[order[i]] / sxe;
			uint32_t j = i;
			while (j < nch && ch_node[order[j]] / sxe == y) j++;
			put_le_dev(b + idx, y - last_y, f.yw); idx += f.yw;
			last_y = y;
			put_le_dev(b + idx, j - i, f.xw); idx += f.xw;
			uint32_t last_x = 0;
			for (uint32_t k = i; k < j; k++) {
				const uint32_t x = ch_node[order[k]] - sxe * y;
				put_le_dev(b + idx, x - last_x, f.xw); idx += f.xw;
				last_x = x;
			}
			i = j;
		}
		f.boc_len[zi] = idx;
		a.n_raw[zi] = total; a.n_valid[zi] = total;
		*s_carry = 0;
	}
	__syncthreads();
	__threadfence_block();
	// an item's code points move by dst - vstart of its chain (wrapping)
	for (uint32_t c = tid; c < nch; c += kEmitBlock) dst[c] -= vstart[c];
	__syncthreads();
	__threadfence_block();

	// ---- expansion to the final place, difference code, store: in windows of wcap words
	const uint32_t nwords = (total + 15u) >> 4, nbytes = (total + 3u) >> 2;
	const uint4* adjm = a.adjm + zi * a.adjm_stride;
	uint8_t* out = f.payload + f.pbase[zi];        // 4-byte aligned
	uint8_t* dcode = f.dcode + a.cbase[zi];        // 16-byte aligned (crack_pass rounds the capacities)
	// the segments to walk stand in the list unless there were too many for it: then whoever meets one walks it.  The
	// walks last as long as the longest segment, so the list's first wavefronts do nothing else and the others share
	// the rest of the items
	const uint32_t nl = *s_nlong;
	const bool listed = nl <= kEmitLong;
	const uint32_t walkers = listed ? min((nl + kWave - 1u) / kWave, static_cast<uint32_t>(kEmitWaves / 2)) * kWave : 0u;      // threads, whole wavefronts
	for (uint32_t w0 = 0; w0 < nwords; w0 += sl.wcap) {
		const uint32_t wn = min(sl.wcap, nwords - w0);
		for (uint32_t i = tid; i < wn; i += kEmitBlock) words[i] = 0u;
		__syncthreads();
		auto or_word = [&](uint32_t gw, uint32_t v) {
			const uint32_t wi = gw - w0;
			if (v && wi < wn) atomicOr(words + wi, v);
		};
		// where item i begins: its raw offset moved with its chain, the last chain that begins at or in front of it (empty
		// chains share their successor's first item)
		auto place = [&](uint32_t i) -> uint32_t {
			uint32_t lo = 0, hi = nch;
			while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (item0[mid] <= i) lo = mid; else hi = mid; }
			return sl.off[i] + dst[lo];
		};
		auto outside = [&](uint32_t p, uint32_t len) -> bool { return (p >> 4) >= w0 + wn || ((p + len - 1u) >> 4) < w0; };
		// a segment too long for its dart's 16 bytes, a loop, the half of a split segment: walked again from its node,
		// 16 code points collected per word
		auto walk = [&](uint32_t d, uint32_t p, uint32_t len) {
			const uint32_t v0 = a.node_vertex[sl.nb + (d >> 2)];
			uint32_t y = v0 / a.sxe, x = v0 - y * a.sxe, k = d & 3u, acc = 0u;
			MicroTile c;
			c.lo = c.hi = make_uint4(0, 0, 0, 0); c.mx = c.my = 0xFFFFFFFFu;
			for (uint32_t s = 0; s < len; s++) {
				const uint32_t g = p + s;
				acc |= trail_code(k) << (2u * (g & 15u));
				if ((g & 15u) == 15u || s + 1u == len) { or_word(g >> 4, acc); acc = 0u; }
				trail_step(x, y, k);
				if (s + 1u == len) break;
				// (a walk never leaves the graph, whose micro-tiles end there; one that would has not written its segment: the
				// slice says so, k_code_offsets reports it and the run ends with the walk's overflow error)
				if (x > a.sx || y > a.sy) { atomicOr(a.slice_err + zi, TRAIL_ERR_CAPACITY); break; }
				if (!c.holds(x, y)) mt_load(c, adjm, x, y, a.mtx2);
				k = (__ffs(c.nib(x, y) & ~(1u << (k ^ 1u))) - 1) & 3u;
			}
		};
		if (tid < walkers) {
			for (uint32_t j = tid; j < nl; j += walkers) {
				const uint32_t i = s_long[j];
				const uint32_t d = sl.items[i] & ~kItemMask, len = sl.dlen[d], p = place(i);
				if (!outside(p, len)) walk(d, p, len);
			}
		}
		else {
			for (uint32_t i = tid - walkers; i < n; i += kEmitBlock - walkers) {
				const uint32_t it = sl.items[i], kind = it & kItemMask;
				if (kind != kItemSeg && kind != kItemCtl) continue;
				const uint32_t p = place(i);
				if (kind == kItemCtl) { or_word(p >> 4, (it & 3u) << (2u * (p & 15u))); or_word((p + 1u) >> 4, ((it >> 2) & 3u) << (2u * ((p + 1u) & 15u))); continue; }
				const uint32_t d = it & ~kItemMask;
				const uint32_t len = sl.dlen[d];
				if (len == 0u || outside(p, len)) continue;
				if (len <= kInlineCodes && a.dart_inline[sl.nb * 4u + d]) {
					const uint4 q4 = a.dart_codes[sl.nb * 4u + d];
					const uint32_t q[4] = { q4.x, q4.y, q4.z, q4.w };
					uint32_t o[5];
					const uint32_t gw = place_codes128(q, len, p, o);
#pragma unroll
					for (uint32_t j = 0; j < 5; j++) or_word(gw + j, o[j]);
				}
				else if (!listed) walk(d, p, len);
			}
		}
		__syncthreads();
		// whole-slice mod-4 difference code on the words (the code in front of the slice's first is 0), then the store
		for (uint32_t i = tid; i < wn; i += kEmitBlock) {
			const uint32_t gw = w0 + i;
			uint32_t enc = packed_code_diff(words[i], i ? words[i - 1] >> 30 : *s_carry);
			if (gw == nwords - 1u && (total & 15u)) enc &= (1u << (2u * (total & 15u))) - 1u;
			if (f.markov) {
				// one byte per difference code for k_markov_hist / k_markov_pack (bytes behind the last code: 0)
				auto spread = [](uint32_t b) -> uint32_t { uint32_t x = (b | (b << 12)) & 0x000F000Fu; return (x | (x << 6)) & 0x03030303u; };
				*reinterpret_cast<uint4*>(dcode + 16ull * gw) = make_uint4(spread(enc & 255u), spread((enc >> 8) & 255u), spread((enc >> 16) & 255u), spread(enc >> 24));
			}
			else if (4u * gw + 4u <= nbytes) reinterpret_cast<uint32_t*>(out)[gw] = enc;
			else for (uint32_t k = 4u * gw; k < nbytes; k++) out[k] = static_cast<uint8_t>(enc >> (8u * (k - 4u * gw)));
		}
		__syncthreads();
		if (tid == 0) *s_carry = words[wn - 1u] >> 30;
		__syncthreads();
	}
	if (tid == 0) f.payload_len[zi] = f.markov ? 0u : nbytes;
}

// (eight wavefronts per SIMD: two workgroups share a CU only while the registers stay within that)
__global__ void __launch_bounds__(kEmitBlock, 8) k_trail_emit(TrailArgs a, FinishArgs f, uint32_t tcap, uint32_t wcap) {
	extern __shared__ uint32_t s_emit[];
	__shared__ uint32_t s_scan[kEmitWaves];
	__shared__ uint32_t s_long[kEmitLong];      // items whose segments are walked
	__shared__ uint32_t s_nlong, s_carry;
	const uint32_t zi = blockIdx.x + a.z0;
	const uint32_t tid = threadIdx.x;
	if (a.slice_err[zi]) {      // uniform; the run ends with this error (check_walk_errors)
		if (tid == 0) { a.n_raw[zi] = 0; a.n_valid[zi] = 0; f.payload_len[zi] = 0; f.boc_len[zi] = 0; }
		return;
	}
	const uint32_t n = a.n_items[zi];
	const uint32_t nch = a.n_chains[zi];
	const uint64_t nb = a.nbase[zi], kb = a.kbase[zi];
	const uint32_t* items = a.items + a.ibase[zi];
	uint32_t* off = a.item_off + a.ibase[zi];
	const uint32_t* dlen = a.dart_len + nb * 4u;
	const uint8_t* dinl = a.dart_inline + nb * 4u;
	if (tid == 0) s_nlong = 0u;
	__syncthreads();

	// ---- offsets (k_trail_offsets): code offset of every item in raw chain order; the segments to walk are listed on the way
	uint32_t total = 0;
	{
		constexpr uint32_t kPer = 4;
		for (uint32_t i0 = 0; i0 < n; i0 += kEmitBlock * kPer) {
			uint32_t len[kPer], cnt = 0;
#pragma unroll
			for (uint32_t q = 0; q < kPer; q++) {
				const uint32_t i = i0 + tid * kPer + q;
				len[q] = 0;
				if (i < n) {
					const uint32_t it = items[i];
					const uint32_t kind = it & kItemMask;
					if (kind == kItemSeg) {
						const uint32_t d = it & ~kItemMask;
						len[q] = dlen[d];
						if (len[q] > kInlineCodes || (len[q] && !dinl[d])) {
							const uint32_t j = atomicAdd(&s_nlong, 1u);
							if (j < kEmitLong) s_long[j] = i;
						}
					}
					else if (kind == kItemCtl) len[q] = 2u;
				}
				cnt += len[q];
			}
			uint32_t v[1] = { cnt }, tot[1];
			block_excl_add<1, kEmitWaves>(v, tot, s_scan);
			uint32_t o = total + v[0];
#pragma unroll
			for (uint32_t q = 0; q < kPer; q++) {
				const uint32_t i = i0 + tid * kPer + q;
				if (i < n) off[i] = o;
				o += len[q];
			}
			total += tot[0];
		}
	}
	__syncthreads();
	__threadfence_block();
	if (total > a.ccap[zi]) {      // uniform
		if (tid == 0) { atomicOr(a.slice_err + zi, TRAIL_ERR_CAPACITY); a.n_raw[zi] = total; a.n_valid[zi] = total; f.payload_len[zi] = 0; f.boc_len[zi] = 0; }
		return;
	}

	// ---- chain tables: start vertex, first item, first raw code offset
	const EmitSlice sl = { zi, n, nch, total, wcap, items, off, dlen, nb };
	uint32_t* words = s_emit + 2u * tcap;
	const uint32_t* g_node = a.chain_node + kb;
	const uint32_t* g_item0 = a.chain_item0 + kb;
	if (nch <= tcap) {      // uniform
		uint32_t* s_item0 = s_emit;
		uint32_t* s_dst = s_emit + tcap;
		uint32_t* s_node = words;
		uint32_t* s_order = words + tcap;
		uint32_t* s_vstart = words + 2u * tcap;
		for (uint32_t c = tid; c < nch; c += kEmitBlock) {
			const uint32_t i0 = g_item0[c];
			s_item0[c] = i0; s_node[c] = g_node[c]; s_vstart[c] = i0 < n ? off[i0] : total;
		}
		__syncthreads();
		emit_chains_and_codes(a, f, sl, words, s_node, s_item0, s_vstart, s_order, s_dst, s_long, &s_nlong, &s_carry);
	}
	else {
		uint32_t* g_vstart = a.chain_off + kb;
		for (uint32_t c = tid; c < nch; c += kEmitBlock) { const uint32_t i0 = g_item0[c]; g_vstart[c] = i0 < n ? off[i0] : total; }
		__syncthreads();
		__threadfence_block();
		emit_chains_and_codes(a, f, sl, words, g_node, g_item0, g_vstart, f.chain_order + kb, f.chain_dst + kb, s_long, &s_nlong, &s_carry);
	}
}

// ------------------------------------------------------------------------------
// markov (src/markov.hpp): context = previous N difference codes, oldest in the
// least-significant base-4 digit; codes before the slice start count as 0.
// ------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t markov_ctx(const uint8_t* d, uint32_t g, int order) {
	uint32_t ctx = 0;
	for (int j = 1; j <= order; j++) {
		const uint32_t v = (g >= static_cast<uint32_t>(j)) ? d[g - j] : 0u;
		ctx |= v << (2 * (order - j));
	}
	return ctx;
}

// gather_statistics (markov.hpp:193-220): stats[ctx][code]++ for every code of every
// slice (the first code of a slice is counted in row 0).  grid = nslices.
// LDS: the workgroup's own histogram (4^order x 4 counters) when it fits (order <= 6),
// flushed once: the global counters see one atomic per non-zero row entry and workgroup
// instead of one per run of equal codes.
__global__ void __launch_bounds__(kBlock) k_markov_hist(
	const uint8_t* __restrict__ dcode, const uint64_t* __restrict__ cbase, const uint32_t* __restrict__ n_valid,
	int order, uint32_t* __restrict__ hist, uint32_t lds_entries
) {
	extern __shared__ uint32_t s_hist[];
	const uint32_t zi = blockIdx.x;
	const uint8_t* d = dcode + cbase[zi];
	const uint32_t n = n_valid[zi];
	const uint32_t entries = 4u << (2 * order);
	const bool local = entries <= lds_entries;
	if (local) {
		for (uint32_t i = threadIdx.x; i < entries; i += kBlock) s_hist[i] = 0;
		__syncthreads();
	}
	uint32_t* target = local ? s_hist : hist;
	constexpr uint32_t kPer = 32;
	// each thread owns 32 consecutive codes and merges equal (row, code) neighbours
	// before touching memory: straight crack runs collapse to one atomic
	for (uint32_t g0 = threadIdx.x * kPer; g0 < n; g0 += kBlock * kPer) {
		uint32_t key = 0xFFFFFFFFu, cnt = 0;
		const uint32_t g1 = g0 + kPer < n ? g0 + kPer : n;
		for (uint32_t g = g0; g < g1; g++) {
			const uint32_t k = markov_ctx(d, g, order) * 4u + d[g];
			if (k == key) cnt++;
			else {
				if (cnt) atomicAdd(target + key, cnt);
				key = k; cnt = 1;
			}
		}
		if (cnt) atomicAdd(target + key, cnt);
	}
	if (local) {
		__syncthreads();
		for (uint32_t i = threadIdx.x; i < entries; i += kBlock) { const uint32_t v = s_hist[i]; if (v) atomicAdd(hist + i, v); }
	}
}

// encode_markov (markov.hpp:422-473): first code raw in 2 bits, then rank codes
// 0 -> `0`, 1 -> `10`, 2 -> `110`, 3 -> `111` (LSB first).  Bit offsets come from
// a block prefix sum of the code lengths; set bits are OR-ed into 32-bit words.
__global__ void __launch_bounds__(kBlock) k_markov_pack(
	const uint8_t* __restrict__ dcode, const uint64_t* __restrict__ cbase, const uint32_t* __restrict__ n_valid,
	int order, const uint8_t* __restrict__ model /* symbol -> rank */,
	const uint64_t* __restrict__ pbase, uint8_t* __restrict__ payload, uint32_t* __restrict__ payload_len
) {
	__shared__ uint32_t s_scan[kWaves];
	const uint32_t zi = blockIdx.x;
	const uint8_t* d = dcode + cbase[zi];
	const uint32_t n = n_valid[zi];
	uint32_t* words = reinterpret_cast<uint32_t*>(payload + pbase[zi]);
	constexpr uint32_t kPer = 8;
	uint32_t carry = 0;
	for (uint32_t tile = 0; tile < n; tile += kBlock * kPer) {
		const uint32_t g0 = tile + threadIdx.x * kPer;
		uint32_t bits[kPer], lens[kPer], tot_len = 0;
#pragma unroll
		for (uint32_t k = 0; k < kPer; k++) {
			const uint32_t g = g0 + k;
			bits[k] = 0; lens[k] = 0;
			if (g < n) {
				if (g == 0) { bits[k] = d[0]; lens[k] = 2; }
				else {
					const uint32_t r = model[markov_ctx(d, g, order) * 4u + d[g]];
					bits[k] = (r == 0) ? 0u : (r == 1) ? 1u : (r == 2) ? 3u : 7u;
					lens[k] = (r == 0) ? 1u : (r == 1) ? 2u : 3u;
				}
			}
			tot_len += lens[k];
		}
		uint32_t v[1] = { tot_len }, tot[1];
		block_excl_add<1>(v, tot, s_scan);
		uint32_t off = carry + v[0];
#pragma unroll
		for (uint32_t k = 0; k < kPer; k++) {
			if (lens[k] && bits[k]) {
				const uint32_t w = off >> 5, sh = off & 31;
				atomicOr(words + w, bits[k] << sh);
				if (sh + lens[k] > 32) atomicOr(words + w + 1, bits[k] >> (32 - sh));
			}
			off += lens[k];
		}
		carry += tot[0];
	}
	if (threadIdx.x == 0) payload_len[zi] = (carry + 7) / 8;
}

// one workgroup: final offset of every slice's codes (exclusive prefix of BOC + payload bytes) and
// what the host needs of them in one buffer: report = [code_len[nslices] | total lo | total hi | errors]
__global__ void __launch_bounds__(kBlock) k_code_offsets(
	const uint32_t* __restrict__ boc_len, const uint32_t* __restrict__ payload_len, const uint32_t* __restrict__ slice_err,
	uint32_t nslices, uint64_t* __restrict__ out_off, uint32_t* __restrict__ report
) {
	__shared__ unsigned long long s_part[kBlock];
	__shared__ uint32_t s_err;
	if (threadIdx.x == 0) s_err = 0;
	const uint32_t per = (nslices + kBlock - 1) / kBlock;
	const uint32_t z0 = threadIdx.x * per, z1 = min(z0 + per, nslices);
	unsigned long long sum = 0;
	uint32_t err = 0;
	for (uint32_t z = z0; z < z1; z++) { sum += static_cast<unsigned long long>(boc_len[z]) + payload_len[z]; err |= slice_err[z]; }
	s_part[threadIdx.x] = sum;
	__syncthreads();
	if (err) atomicOr(&s_err, err);
	if (threadIdx.x == 0) {
		unsigned long long run = 0;
		for (uint32_t i = 0; i < kBlock; i++) { const unsigned long long v = s_part[i]; s_part[i] = run; run += v; }
		report[nslices] = static_cast<uint32_t>(run); report[nslices + 1] = static_cast<uint32_t>(run >> 32);
	}
	__syncthreads();
	unsigned long long off = s_part[threadIdx.x];
	for (uint32_t z = z0; z < z1; z++) {
		const uint32_t len = boc_len[z] + payload_len[z];
		out_off[z] = off;
		report[z] = len;
		off += len;
	}
	if (threadIdx.x == 0) report[nslices + 2] = s_err;
}

// grid = nslices: copy each slice's BOC index and payload to their final offsets
__global__ void __launch_bounds__(kBlock) k_gather_codes(
	const uint8_t* __restrict__ boc, const uint64_t* __restrict__ bbase, const uint32_t* __restrict__ boc_len,
	const uint8_t* __restrict__ payload, const uint64_t* __restrict__ pbase, const uint32_t* __restrict__ payload_len,
	const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out
) {
	const uint32_t zi = blockIdx.x;
	uint8_t* o = out + out_off[zi];
	const uint32_t nb = boc_len[zi], np = payload_len[zi];
	const uint8_t* b = boc + bbase[zi];
	const uint8_t* p = payload + pbase[zi];
	for (uint32_t i = threadIdx.x; i < nb; i += kBlock) o[i] = b[i];
	for (uint32_t i = threadIdx.x; i < np; i += kBlock) o[nb + i] = p[i];
}

// n bytes from src to dst, any alignment on either side: the device-resident copy of the assembled stream
// (ckl_encoder_keep_device_stream) takes its two bulky sections from buffers of this session.  A device-to-device
// ---- crc32c of a device buffer (the flat label section: header.hpp / crackle.hpp:171-216 store it behind the crack codes) ----
// The register's journey is linear over GF(2): state(c, M) = c * x^bits(M) + state(0, M).  The n bytes are laid right-aligned
// into a frame of G * 256 * P bytes (G a power of two; zeros in front leave a zero register where it is), every thread
// runs its P bytes from a zero register through the byte table, and the pieces are folded pairwise with x^(bits of the
// right half) — inside the workgroups here, over the workgroups in k_crc32c_fold.
struct CrcShifts { uint32_t x[8]; };      // x[k] = x^(8 * piece * 2^k) mod P, reflected representation (ckl_common.hpp: gf_xpow)
__global__ void __launch_bounds__(kBlock) k_crc32c_pieces(const uint8_t* __restrict__ data, uint64_t n, uint64_t pad, uint32_t P, CrcShifts sh, uint32_t* __restrict__ parts) {
	__shared__ uint32_t s_tab[256];
	__shared__ uint32_t s_st[kBlock];
	{
		uint32_t c = threadIdx.x;
		for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ dev::kCrcPoly : (c >> 1);
		s_tab[threadIdx.x] = c;
	}
	__syncthreads();
	const uint64_t f0 = (static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x) * P;      // my piece's place in the frame
	uint32_t c = 0;
	for (uint32_t g = 0; g < P; g += 16) {
		const int64_t m0 = static_cast<int64_t>(f0 + g) - static_cast<int64_t>(pad);           // ... and in the message
		uint32_t w[4] = { 0, 0, 0, 0 };
		if (m0 >= 0 && static_cast<uint64_t>(m0) + 16u <= n) __builtin_memcpy(w, data + m0, 16);      // (unaligned 16-byte load)
		else if (m0 + 16 > 0) for (int b = 0; b < 16; b++) { const int64_t i = m0 + b; if (i >= 0 && static_cast<uint64_t>(i) < n) w[b >> 2] |= static_cast<uint32_t>(data[i]) << (8 * (b & 3)); }
#pragma unroll
		for (int b = 0; b < 16; b++) c = s_tab[(c ^ (w[b >> 2] >> (8 * (b & 3)))) & 0xFFu] ^ (c >> 8);
	}
	s_st[threadIdx.x] = c;
	__syncthreads();
	for (int k = 0; k < 8; k++) {
		const uint32_t stride = 1u << k;
		if ((threadIdx.x & (2u * stride - 1u)) == 0u) s_st[threadIdx.x] = gf_mul(s_st[threadIdx.x], sh.x[k]) ^ s_st[threadIdx.x + stride];
		__syncthreads();
	}
	if (threadIdx.x == 0) parts[blockIdx.x] = s_st[0];
}
// one workgroup: the G (a power of two, <= kBlock) workgroup states -> the finished crc32c (register preset to all ones, inverted at the end)
__global__ void __launch_bounds__(kBlock) k_crc32c_fold(const uint32_t* __restrict__ parts, uint32_t G, CrcShifts sh, uint32_t init_term, uint32_t* __restrict__ out) {
	__shared__ uint32_t s_st[kBlock];
	s_st[threadIdx.x] = threadIdx.x < G ? parts[threadIdx.x] : 0u;
	__syncthreads();
	for (int k = 0; (1u << k) < G; k++) {
		const uint32_t stride = 1u << k;
		if ((threadIdx.x & (2u * stride - 1u)) == 0u && threadIdx.x + stride < G) s_st[threadIdx.x] = gf_mul(s_st[threadIdx.x], sh.x[k]) ^ s_st[threadIdx.x + stride];
		__syncthreads();
	}
	if (threadIdx.x == 0) out[0] = ~(s_st[0] ^ init_term);
}

// hipMemcpyAsync moved the 13 MB of C2's crack codes at 115 GB/s (113 us on the encode's tail); this is a plain
// streaming kernel.  Destination words are written aligned; a source word is two aligned loads and a funnel shift.
// grid-stride, block = kBlock.
__global__ void __launch_bounds__(kBlock) k_copy_bytes(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint64_t n) {
	const uint64_t head = min(n, static_cast<uint64_t>((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));      // bytes in front of dst's first aligned word
	const uint64_t words = (n - head) / 4u;
	const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
	const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
	if (tid < head) dst[tid] = src[tid];
	const uint64_t tail0 = head + words * 4u;
	if (tid < n - tail0) dst[tail0 + tid] = src[tail0 + tid];
	const uint8_t* s0 = src + head;
	const uint32_t sh = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(s0) & 3u) * 8u;
	const uint32_t* sw = reinterpret_cast<const uint32_t*>(reinterpret_cast<uintptr_t>(s0) & ~static_cast<uintptr_t>(3));
	uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
	if (sh == 0u) {
		for (uint64_t i = tid; i < words; i += stride) dw[i] = sw[i];
	}
	else {
		// (the last word's second load reads the aligned word that holds the source's last bytes: inside the buffer)
		for (uint64_t i = tid; i < words; i += stride) dw[i] = __funnelshift_r(sw[i], sw[i + 1], sh);
	}
}

// grid = slices, block = kBlock: the walk's events of a slice by kind, and the longest run of events that take no decision
// (a node with one remaining edge is left by it, a dead end returns: kEvSeg / kEvDead / kEvEnd; only kEvBseg picks an edge
// AND leaves one behind).  counts: [slices][5] = seg, bseg, dead, end, longest run without a kEvBseg
__global__ void __launch_bounds__(kBlock) k_trail_step_kinds(const uint32_t* __restrict__ events, const uint64_t* __restrict__ ibase, const uint32_t* __restrict__ n_events, uint32_t* __restrict__ counts) {
	__shared__ uint32_t s_c[5];
	const uint32_t zi = blockIdx.x;
	if (threadIdx.x < 5) s_c[threadIdx.x] = 0u;
	__syncthreads();
	const uint32_t n = n_events[zi] & ~(dev::kEvFormatAddr12 | dev::kEvWalkWide);
	const uint32_t* ev = events + ibase[zi];
	uint32_t c[4] = { 0, 0, 0, 0 };
	for (uint32_t i = threadIdx.x; i < n; i += kBlock) c[ev[i] >> 30]++;
	for (int k = 0; k < 4; k++) if (c[k]) atomicAdd(&s_c[k], c[k]);
	if (threadIdx.x == 0) {      // (one thread: a diagnostic, not a product path)
		uint32_t run = 0, longest = 0;
		for (uint32_t i = 0; i < n; i++) { if ((ev[i] >> 30) == 1u) run = 0; else { run++; longest = run > longest ? run : longest; } }
		s_c[4] = longest;
	}
	__syncthreads();
	if (threadIdx.x < 5) counts[zi * 5u + threadIdx.x] = s_c[threadIdx.x];
}

}  // namespace ckl

// ------------------------------------------------------------------------------
// host orchestration
// ------------------------------------------------------------------------------
using namespace ckl;

// crc32c of n > 0 device bytes into out[0], on stream s (parts: scratch of kBlock words)
static void crc32c_device(const uint8_t* data, uint64_t n, uint32_t* parts, uint32_t* out, hipStream_t s) {
	uint32_t P = 128, G = 1;
	while (G < static_cast<uint32_t>(kBlock) && static_cast<uint64_t>(G) * kBlock * P < n) G <<= 1;
	if (static_cast<uint64_t>(G) * kBlock * P < n) P = static_cast<uint32_t>(((n + static_cast<uint64_t>(G) * kBlock - 1) / (static_cast<uint64_t>(G) * kBlock) + 15) / 16 * 16);
	const uint64_t frame = static_cast<uint64_t>(G) * kBlock * P;
	// (the sixteen powers depend on the piece length only — 128 bytes for every section up to 8 MB — and cost the host ~40 us,
	// on the encode's tail: kept from call to call)
	static std::mutex shifts_mutex;
	static uint32_t shifts_for = 0;
	static CrcShifts shifts_in, shifts_over;
	CrcShifts in_wg, over_wg;
	{
		std::lock_guard<std::mutex> lock(shifts_mutex);
		if (shifts_for != P) {
			for (int k = 0; k < 8; k++) {
				shifts_in.x[k] = gf_xpow(8ull * P << k);
				shifts_over.x[k] = gf_xpow(8ull * P * kBlock << k);
			}
			shifts_for = P;
		}
		in_wg = shifts_in; over_wg = shifts_over;
	}
	hipLaunchKernelGGL(k_crc32c_pieces, dim3(G), dim3(kBlock), 0, s, data, n, frame - n, P, in_wg, parts);
	hipLaunchKernelGGL(k_crc32c_fold, dim3(1), dim3(kBlock), 0, s, parts, G, over_wg, gf_mul(0xFFFFFFFFu, gf_xpow(8ull * n)), out);
}

// k_copy_bytes on stream s
static void copy_bytes_device(const uint8_t* src, uint8_t* dst, uint64_t n, hipStream_t s) {
	if (!n) return;
	const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((n / 4u + kBlock - 1) / kBlock + 1u, 8192u));
	hipLaunchKernelGGL(k_copy_bytes, dim3(blocks), dim3(kBlock), 0, s, src, dst, n);
}

namespace {

// Many small tables in ONE copy: the tables become views of a packed block (a copy of a few bytes costs
// ~8 us of stream time, and crack_pass needs fifteen of them between two kernels of the trail).
struct UploadPacker {
	struct Item { void* buf; size_t off, count; void (*bind)(void*, uint8_t*, size_t); };
	std::vector<Item> items;
	std::vector<uint8_t> image;
	template <typename T>
	void add(DevBuf<T>& dst, const std::vector<T>& src) {
		const size_t off = (image.size() + 255) & ~static_cast<size_t>(255);
		image.resize(off + std::max<size_t>(src.size(), 1) * sizeof(T));
		if (!src.empty()) memcpy(image.data() + off, src.data(), src.size() * sizeof(T));
		items.push_back({ &dst, off, src.size(), [](void* b, uint8_t* base, size_t n) { static_cast<DevBuf<T>*>(b)->borrow(reinterpret_cast<T*>(base), n); } });
	}
	// `block` must not be in use by kernels of another stream; the copy is ordered on `s`
	// staging: the session's pinned host block for this image (kept until its next commit: the copy kernel reads it), or null
	void commit(DevBuf<uint8_t>& block, hipStream_t s, void** staging = nullptr) {
		if (image.empty()) return;
		for (const Item& it : items) it.bind(it.buf, nullptr, 0);        // views of the old block go first: ensure() may free it
		block.ensure(image.size());
		if (staging) {
			if (*staging) host_out_free(*staging);
			*staging = host_out_alloc(std::max<size_t>(image.size(), 64u << 10));      // >= 64 KiB: pinned
			memcpy(*staging, image.data(), image.size());
			upload_small(block.p, *staging, image.size(), s, *staging);
		}
		else CKL_HIP(hipMemcpyAsync(block.p, image.data(), image.size(), hipMemcpyHostToDevice, s));      // pageable source: staged before the call returns
		for (const Item& it : items) it.bind(it.buf, block.p + it.off, it.count);
	}
};

template <typename LABEL>
VolumeStats volume_stats(ckl_encoder& e, const LABEL* labels, uint64_t voxels) {
	VolumeStats st;
	if (voxels == 0) return st;
	hipStream_t s = e.stream;
	e.d_stats.ensure(2);
	CKL_HIP(hipMemsetAsync(e.d_stats.p, 0, 2 * sizeof(unsigned long long), s));
	const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((voxels + kBlock - 1) / kBlock, 256ull * 8));
	hipLaunchKernelGGL(k_stats<LABEL>, dim3(blocks), dim3(kBlock), 0, s, labels, voxels, e.d_stats.p);
	auto r = download(e.d_stats.p, 2, s);
	st.max_label = r[0]; st.pairs = r[1];
	LABEL f, l;
	CKL_HIP(hipMemcpy(&f, labels, sizeof(LABEL), hipMemcpyDeviceToHost));
	CKL_HIP(hipMemcpy(&l, labels + (voxels - 1), sizeof(LABEL), hipMemcpyDeviceToHost));
	st.first = f; st.last = l;
	return st;
}

// ckl_encoder_stats left the planes of exactly this volume behind (single use: the callers clear planes_for)
inline bool planes_cached(const ckl_encoder& e, const void* labels, int64_t sx, int64_t sy, int64_t sz) {
	return e.planes_for == labels && e.planes_dims[0] == sx && e.planes_dims[1] == sy && e.planes_dims[2] == sz;
}

// crack edges of slice zi, exactly: the interior pixel pairs that differ (IMPERMISSIBLE) or are equal (PERMISSIBLE)
inline uint64_t crack_edges(const ckl_encoder& e, int64_t sx, int64_t sy, size_t zi, bool permissible) {
	const uint64_t interior = static_cast<uint64_t>(sx > 0 ? sx - 1 : 0) * sy + static_cast<uint64_t>(sx) * (sy > 0 ? sy - 1 : 0);
	const uint64_t differ = static_cast<uint64_t>(e.count_v[zi]) + e.count_h[zi];
	return permissible ? interior - differ : differ;
}

// the fast planes kernel's per-slice counts -> e.count_v / count_h and the volume's statistics
void planes_collect(ckl_encoder& e, uint32_t ns, VolumeStats* st, const std::vector<unsigned long long>* fetched = nullptr) {
	std::vector<unsigned long long> mine;
	if (!fetched) { mine = download(e.d_plane_out.p, 4ull * ns, e.stream); fetched = &mine; }
	const std::vector<unsigned long long>& o = *fetched;
	e.count_v.resize(ns); e.count_h.resize(ns);
	VolumeStats v;
	for (uint32_t zi = 0; zi < ns; zi++) {
		e.count_v[zi] = static_cast<uint32_t>(o[4ull * zi]);
		e.count_h[zi] = static_cast<uint32_t>(o[4ull * zi + 1]);
		v.pairs += o[4ull * zi + 2];
		v.max_label = std::max<uint64_t>(v.max_label, o[4ull * zi + 3]);
	}
	e.planes_deferred = false;
	if (st) *st = v;
}

// The trail's zero fills (slice errors, counters, chain start bits) depend on the dimensions only.  On the
// label stream, which is idle until the walk, they run beside the planes kernel instead of between the node
// counts and k_trail_nodes (3 fills, 25 us + their launch gaps at C2).  crack_pass waits for ev_prezero.
void trail_prezero(ckl_encoder& e, int64_t sx, int64_t sy, int64_t sz) {
	hipStream_t s = e.stream2;
	const uint32_t ns = static_cast<uint32_t>(sz);
	const uint64_t nverts = static_cast<uint64_t>(sx + 1) * (sy + 1);
	const uint32_t start_words = static_cast<uint32_t>((nverts + 31) / 32);
	e.d_slice_err.ensure(ns);
	e.t_counters.ensure(7 * static_cast<size_t>(ns));
	e.t_start_bits.ensure(static_cast<size_t>(start_words) * ns);
	CKL_HIP(hipMemsetAsync(e.d_slice_err.p, 0, ns * sizeof(uint32_t), s));
	CKL_HIP(hipMemsetAsync(e.t_counters.p, 0, 7 * static_cast<size_t>(ns) * sizeof(uint32_t), s));
	CKL_HIP(hipMemsetAsync(e.t_start_bits.p, 0, static_cast<size_t>(start_words) * ns * sizeof(uint32_t), s));
	CKL_HIP(hipEventRecord(e.ev_prezero, s));
	e.trail_zeroed = true;
}

// One pass over the labels -> the two "differs from neighbour" bit planes and their
// per-slice population counts (exact crack edge and run counts follow from these) and,
// on the fast path, the whole-volume reductions of lib.hpp:224-256 from the same read.
template <typename LABEL>
void planes_pass(ckl_encoder& e, const LABEL* labels, int64_t sx, int64_t sy, int64_t sz, VolumeStats* st, bool defer = false) {
	hipStream_t s = e.stream;
	const uint32_t ns = static_cast<uint32_t>(sz);
	e.trail_zeroed = false;
	e.planes_deferred = false;
	e.row_words = static_cast<uint32_t>((sx + 31) / 32);
	e.plane_words = static_cast<uint64_t>(e.row_words) * sy;
	e.d_planes.ensure(2 * e.plane_words * ns);
	constexpr uint32_t P = 16 / sizeof(LABEL);
	const bool fast = !getenv("CKL_PLANES_GENERIC") && sx >= static_cast<int64_t>(P) && sx % P == 0 && (reinterpret_cast<uintptr_t>(labels) & 15u) == 0;
	if (fast) {
		const uint32_t strips = static_cast<uint32_t>((sx + 64 * P - 1) / (64 * P));
		const uint32_t bands = static_cast<uint32_t>((sy + kBandRows - 1) / kBandRows);
		const uint32_t nblk = (strips * bands + kWaves - 1) / kWaves;
		e.d_plane_partial.ensure(4ull * nblk * ns);
		e.d_plane_partial_max.ensure(static_cast<size_t>(nblk) * ns);
		e.d_plane_out.ensure(4ull * ns + 1);
		trail_prezero(e, sx, sy, sz);
		hipLaunchKernelGGL(k_label_planes_stream<LABEL>, dim3(nblk, ns), dim3(kBlock), 0, s,
			labels, static_cast<uint32_t>(sx), static_cast<uint32_t>(sy), strips, bands,
			plane_v(e), plane_h(e, ns), e.row_words, e.plane_words,
			e.d_plane_partial.p, e.d_plane_partial_max.p, e.d_plane_out.p + 4ull * ns);
		hipLaunchKernelGGL(k_planes_reduce, dim3(ns), dim3(kBlock), 0, s, e.d_plane_partial.p, e.d_plane_partial_max.p, nblk, e.d_plane_out.p, e.d_plane_out.p + 4ull * ns);
		// deferred: graph_pass fetches the counts together with its own (k_trail_graph decides the crack
		// format from the device's pair count: one host round trip less in front of it)
		e.planes_deferred = defer;
		if (!e.planes_deferred) planes_collect(e, ns, st);
		return;
	}
	if (st) *st = volume_stats<LABEL>(e, labels, static_cast<uint64_t>(sx) * sy * sz);
	e.d_count_vh.ensure(2 * static_cast<size_t>(ns));
	CKL_HIP(hipMemsetAsync(e.d_count_vh.p, 0, 2 * static_cast<size_t>(ns) * sizeof(uint32_t), s));
	const uint32_t chunks = static_cast<uint32_t>((sx + 63) / 64);
	const uint64_t units = static_cast<uint64_t>(chunks) * sy;
	hipLaunchKernelGGL(k_label_planes<LABEL>, dim3(static_cast<uint32_t>((units + kWaves * kPlaneUnroll - 1) / (kWaves * kPlaneUnroll)), ns), dim3(kBlock), 0, s,
		labels, static_cast<uint32_t>(sx), static_cast<uint32_t>(sy), chunks,
		plane_v(e), plane_h(e, ns), e.row_words, e.plane_words,
		e.d_count_vh.p, e.d_count_vh.p + ns);
	std::vector<uint32_t> c = download(e.d_count_vh.p, 2 * static_cast<size_t>(ns), s);
	e.count_v.assign(c.begin(), c.begin() + ns);
	e.count_h.assign(c.begin() + ns, c.end());
}

// planes_pass for the session's label width
void planes_pass_any(ckl_encoder& e, const void* labels, int64_t sx, int64_t sy, int64_t sz, VolumeStats* st) {
	with_label_type(e.dtype_bytes, [&](auto t) { planes_pass(e, static_cast<const typename decltype(t)::type*>(labels), sx, sy, sz, st); });
}

// crack graph (vertex nibbles in tiles, crackcodes.hpp:66-125) + the node / corner counts
// of the trail graph (ckl_trail.hpp)
// ON_DEVICE: decided on the device from the planes kernel's pair count (crackle.hpp:50-55; needs planes_deferred);
// `st` receives the deferred statistics
enum class GraphFormat : uint32_t { IMPERMISSIBLE = 0, PERMISSIBLE = 1, ON_DEVICE = 2 };      // (the values are k_trail_graph's)
inline GraphFormat graph_format(bool permissible) { return permissible ? GraphFormat::PERMISSIBLE : GraphFormat::IMPERMISSIBLE; }
void graph_pass(ckl_encoder& e, int64_t sx, int64_t sy, int64_t sz, GraphFormat format, VolumeStats* st = nullptr) {
	hipStream_t s = e.stream;
	const uint32_t ns = static_cast<uint32_t>(sz);
	e.tiles_x = static_cast<uint32_t>((sx + 1 + kTrailTileDim - 1) / kTrailTileDim);
	e.tiles_y = static_cast<uint32_t>((sy + 1 + 7) / 8);      // rows of 32 x 8 pieces
	// micro-tiles of 8 x 8 vertices, 32 bytes (2 uint4) each, 2 x 2 of them per 128-byte line
	const uint32_t mtx = static_cast<uint32_t>((sx + 1 + 7) / 8), mty = static_cast<uint32_t>((sy + 1 + 7) / 8);
	e.mtx2 = (mtx + 1) / 2;
	e.adjm_stride = static_cast<uint64_t>(e.mtx2) * ((mty + 1) / 2) * 4 * 2;      // uint4 per slice
	e.d_adjm.ensure(e.adjm_stride * ns);
	e.graph_blocks = (e.tiles_x * e.tiles_y + kBlock - 1) / kBlock;
	e.t_blk_special.ensure(static_cast<size_t>(e.graph_blocks) * ns);
	e.t_blk_corner.ensure(static_cast<size_t>(e.graph_blocks) * ns);
	e.d_count_vh.ensure(4 * static_cast<size_t>(ns));
	const bool on_device = format == GraphFormat::ON_DEVICE;
	if (on_device && !e.planes_deferred) throw Error(CKL_ERR_RUNTIME, "crackle_amd: internal: crack format left to the device without deferred counts");
	const unsigned long long half_voxels = static_cast<unsigned long long>(static_cast<int64_t>(static_cast<uint64_t>(sx) * sy * sz) / 2);
	hipLaunchKernelGGL(k_trail_graph, dim3(e.graph_blocks, ns), dim3(kBlock), 0, s,
		plane_v(e), plane_h(e, ns), e.row_words, e.plane_words,
		static_cast<uint32_t>(sx), static_cast<uint32_t>(sy), static_cast<uint32_t>(format),
		on_device ? e.d_plane_out.p + 4ull * ns : nullptr, half_voxels,
		reinterpret_cast<uint32_t*>(e.d_adjm.p), e.adjm_stride * 4,
		e.mtx2, e.tiles_x, e.tiles_y, e.t_blk_special.p, e.t_blk_corner.p);
	hipLaunchKernelGGL(k_trail_count_scan, dim3(ns), dim3(kBlock), 0, s, e.t_blk_special.p, e.t_blk_corner.p, e.graph_blocks,
		e.d_count_vh.p + 2 * static_cast<size_t>(ns), e.d_count_vh.p + 3 * static_cast<size_t>(ns));
	std::vector<unsigned long long> po;
	if (e.planes_deferred) {
		po.resize(4ull * ns);
		CKL_HIP(hipMemcpyAsync(po.data(), e.d_plane_out.p, po.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
	}
	std::vector<uint32_t> c = download(e.d_count_vh.p + 2 * static_cast<size_t>(ns), 2 * static_cast<size_t>(ns), s);
	e.count_special.assign(c.begin(), c.begin() + ns);
	e.count_corner.assign(c.begin() + ns, c.end());
	VolumeStats v;
	if (!po.empty()) planes_collect(e, ns, &v, &po);
	if (st && !po.empty()) *st = v;
	e.graph_permissible = on_device ? static_cast<int64_t>(v.pairs) < static_cast<int64_t>(static_cast<uint64_t>(sx) * sy * sz) / 2 : format == GraphFormat::PERMISSIBLE;
}

// What a crack pass is asked for.  HISTOGRAM stops behind k_markov_hist (markov_order > 0): the trail stays on the
// device.  CODES goes on through the packing, the gather and the report: the codes stay in e.d_codes_out.
enum class CrackGoal { HISTOGRAM, CODES };
struct CrackRequest {
	CrackGoal goal = CrackGoal::CODES;
	bool permissible = false;
	int markov_order = 0;
	const std::vector<uint8_t>* model = nullptr;      // the forced model (symbol -> rank); null: from this volume's histogram
	bool reuse_trail = false;                          // the trail of a HISTOGRAM pass over the same planes is still there: only pack it
	std::function<void()> overlap;                     // the label side: runs on the host while the trail kernels execute
};
struct CrackResult {
	std::vector<uint32_t> code_len;     // per slice: boc + payload bytes
	uint64_t total = 0;                 // bytes of all crack codes; they stay in e.d_codes_out
	bool any_chain = false;
	std::vector<uint32_t> hist;         // markov histogram (unless a model was forced)
	std::vector<uint8_t> model;         // the model the codes were packed under
};

// Dynamic LDS of k_trail_walk for slices of up to `max_special` nodes (+ what k_trail_loops / _components add)
inline size_t trail_walk_lds(uint32_t max_special) { return (static_cast<size_t>(max_special) + 256) * 16 + 1024; }

// Whether k_trail_emit takes the place of k_trail_offsets + k_trail_expand + k_finish for a volume, and with how much LDS.
// Decided before the launch from what the host has: the crack edges of the largest slice and the largest chain
// capacity.  A slice's code points are its crack edges plus two per 'b' and 't'; the word buffer is sized for an eighth
// more than the edges (a slice with more is emitted in windows: correct, slower).  Static and dynamic LDS together stay
// within kEmitLdsCap, so that two workgroups share a CU; a volume whose largest slice asks for more takes the three kernels.
// CKL_TRAIL_EMIT=0 forces the three kernels; CKL_TRAIL_EMIT_LDS=n (testing) puts n bytes in kEmitLdsCap's place;
// CKL_TRAIL_EMIT_WORDS=n (testing) shrinks the word buffer to n words, so that small slices are emitted in windows too.
constexpr size_t kEmitLdsCap = 80 * 1024;
struct EmitPlan {
	bool fused = false;
	uint32_t tcap = 0, wcap = 0;      // chains staged in LDS, words of code points
	size_t dyn = 0, need = 0;         // dynamic LDS in bytes; static + dynamic
};
EmitPlan emit_plan(uint64_t max_edges, uint32_t max_kcap, int max_lds) {
	EmitPlan p;
	static const size_t static_lds = [] {      // the kernel's own arrays: asked once (the same code object on every device)
		hipFuncAttributes fattr;
		CKL_HIP(hipFuncGetAttributes(&fattr, reinterpret_cast<const void*>(&k_trail_emit)));
		return static_cast<size_t>(fattr.sharedSizeBytes);
	}();
	p.tcap = std::min<uint32_t>(kFinishChains, ((max_kcap + 15u) / 16u) * 16u);
	const uint64_t words = (max_edges + max_edges / 8 + 1024 + 15) / 16;
	p.wcap = static_cast<uint32_t>(std::min<uint64_t>(words, 1u << 28));
	if (const char* env = getenv("CKL_TRAIL_EMIT_WORDS")) p.wcap = static_cast<uint32_t>(std::max(1, std::min<int>(atoi(env), static_cast<int>(p.wcap))));      // testing: windows
	p.dyn = 4 * (2 * static_cast<size_t>(p.tcap) + std::max<size_t>(3 * static_cast<size_t>(p.tcap), p.wcap));
	p.need = static_lds + p.dyn;
	size_t cap = kEmitLdsCap;
	if (const char* env = getenv("CKL_TRAIL_EMIT_LDS")) cap = static_cast<size_t>(std::max(0, atoi(env)));
	cap = std::min(cap, static_cast<size_t>(std::max(0, max_lds)));
	const char* sw = getenv("CKL_TRAIL_EMIT");
	p.fused = !(sw && !strcmp(sw, "0")) && words < (1u << 28) && p.need <= cap;
	return p;
}

// k_finish's view of the session (the arrays are there: crack_pass has sized them)
FinishArgs finish_args(const ckl_encoder& e, int64_t sx, int64_t sy, int markov_order) {
	FinishArgs fa;
	fa.sx = static_cast<int>(sx); fa.sy = static_cast<int>(sy);
	fa.xw = byte_width(static_cast<uint64_t>(sx) + 1); fa.yw = byte_width(static_cast<uint64_t>(sy) + 1);
	fa.markov = markov_order ? 1u : 0u;
	fa.cbase = e.d_cbase.p; fa.kbase = e.d_kbase.p;
	fa.n_chains = e.d_n_chains.p; fa.n_raw = e.d_n_raw.p; fa.n_valid = e.d_n_valid.p;
	fa.cp = e.d_cp.p; fa.chain_node = e.d_chain_node.p; fa.chain_off = e.d_chain_off.p; fa.chain_clen = e.d_chain_clen.p;
	fa.chain_order = e.d_chain_order.p; fa.chain_dst = e.d_chain_dst.p; fa.chain_vstart = e.d_chain_vstart.p;
	fa.fcode = e.d_fcode.p; fa.dcode = e.d_dcode.p;
	fa.pbase = e.d_pbase.p; fa.payload = e.d_payload.p; fa.bbase = e.d_bbase.p; fa.boc = e.d_boc.p;
	fa.payload_len = e.d_payload_len.p; fa.boc_len = e.d_boc_len.p;
	fa.z0 = 0;
	return fa;
}

// the trail kernels' view of the session (ckl_trail.hpp), with the walk's test switches; dbg stays null
TrailArgs trail_args(const ckl_encoder& e, int64_t sx, int64_t sy, uint32_t ns) {
	const uint64_t nverts = static_cast<uint64_t>(sx + 1) * (sy + 1);
	TrailArgs ta;
	ta.adjm = e.d_adjm.p; ta.adjm_stride = e.adjm_stride; ta.mtx2 = e.mtx2; ta.tiles_x = e.tiles_x; ta.tiles_y = e.tiles_y;
	ta.planeV = plane_v(e); ta.planeH = plane_h(e, ns); ta.row_words = e.row_words; ta.plane_words = e.plane_words;
	ta.sx = static_cast<uint32_t>(sx); ta.sy = static_cast<uint32_t>(sy); ta.inv = e.graph_permissible ? 0xFFFFFFFFu : 0u;
	ta.sxe = static_cast<uint32_t>(sx + 1); ta.sye = static_cast<uint32_t>(sy + 1); ta.nverts = static_cast<uint32_t>(nverts);
	ta.max_steps = e.t_max_steps.p;
	ta.nbase = e.t_nbase.p; ta.ncap = e.t_ncap.p;
	ta.n_nodes = e.t_counters.p; ta.n_corners = e.t_counters.p + 2 * ns;
	ta.n_starts = e.t_counters.p + 3 * ns; ta.n_items = e.t_counters.p + 4 * ns;
	ta.node_vertex = e.t_node_vertex.p; ta.node_adj = e.t_node_adj.p; ta.vert2node = e.t_vert2node.p;
	ta.cobase = e.t_cobase.p; ta.cocap = e.t_cocap.p; ta.corner_vertex = e.t_corner_vertex.p;
	ta.dart_end = e.t_dart_end.p; ta.dart_len = e.t_dart_len.p; ta.dart_minv = e.t_dart_minv.p; ta.dart_minpos = e.t_dart_minpos.p;
	ta.dart_codes = e.t_dart_codes.p; ta.dart_inline = e.t_dart_inline.p;
	ta.parent = e.t_parent.p; ta.compmin = e.t_compmin.p;
	ta.start_bits = e.t_start_bits.p; ta.start_words = static_cast<uint32_t>((nverts + 31) / 32); ta.starts = e.t_starts.p;
	ta.ibase = e.t_ibase.p; ta.icap = e.t_icap.p; ta.items = e.t_items.p; ta.item_off = e.t_item_off.p;
	ta.sbase = e.d_sbase.p; ta.scap = e.d_scap.p; ta.stack_node = e.d_stack_node.p; ta.stack_item = e.d_stack_code.p;
	ta.kbase = e.d_kbase.p; ta.kcap = e.d_kcap.p;
	ta.chain_node = e.d_chain_node.p; ta.chain_item0 = e.t_chain_item0.p; ta.chain_off = e.d_chain_off.p; ta.chain_clen = e.d_chain_clen.p;
	ta.n_chains = e.d_n_chains.p; ta.n_raw = e.d_n_raw.p; ta.n_valid = e.d_n_valid.p;
	ta.cbase = e.d_cbase.p; ta.ccap = e.d_ccap.p; ta.cp = e.d_cp.p; ta.slice_err = e.d_slice_err.p;
	ta.events = e.t_events.p; ta.n_events = e.t_counters.p + 5 * ns; ta.seg_len_sum = e.t_counters.p + 6 * ns; ta.chain_ev0 = e.t_chain_ev0.p; ta.ev_lnd = e.t_ev_lnd.p; ta.ev_item = e.t_ev_item.p;
	ta.dbg = nullptr;
	{ const char* env = getenv("CKL_TRAIL_WALK"); ta.walk_plain = (env && !strcmp(env, "plain")) ? 1u : 0u; ta.walk_no_regs = (env && !strcmp(env, "lds")) ? 1u : 0u; }
	{ const char* env = getenv("CKL_TRAIL_WALK_STACK"); ta.walk_stack_cap = env ? static_cast<uint32_t>(std::max(1, atoi(env))) : 0xFFFFFFFFu; }
	ta.graph_blocks = e.graph_blocks; ta.blk_special = e.t_blk_special.p; ta.blk_corner = e.t_blk_corner.p;
	ta.z0 = 0;
	return ta;
}

// CKL_TRAIL_DIAG on a tuning build: what the trail's kernels counted (ta_dbg: TrailArgs::dbg, or null)
void trail_diag(ckl_encoder& e, uint32_t ns, const unsigned long long* ta_dbg, uint32_t max_special, size_t trail_lds_used) {
	hipStream_t s = e.stream;
	std::vector<uint32_t> c = download(e.t_counters.p, 5 * static_cast<size_t>(ns), s);
	double m[5] = { 0 };
	for (int k = 0; k < 5; k++) for (uint32_t zi = 0; zi < ns; zi++) m[k] += static_cast<double>(c[static_cast<size_t>(k) * ns + zi]) / ns;
	double sp = 0, co = 0;
	for (uint32_t zi = 0; zi < ns; zi++) { sp += static_cast<double>(e.count_special[zi]) / ns; co += static_cast<double>(e.count_corner[zi]) / ns; }
	if (ta_dbg) {
		std::vector<unsigned long long> g = download(ta_dbg, 16, s);
		if (g[11]) fprintf(stderr, "[ckl trail diag, k_trail_walk] mean cycles per slice: table fill=%.0f fill + walk=%.0f\n", static_cast<double>(g[6]) / g[11], static_cast<double>(g[7]) / g[11]);
		if (g[11]) fprintf(stderr, "[ckl trail diag, k_trail_walk] slices=%llu iterations/slice=%.0f cycles/iteration=%.0f clock=%.2f GHz (cycles / 100 MHz ticks)\n",
			g[11], static_cast<double>(g[8]) / g[11], g[8] ? static_cast<double>(g[9]) / g[8] : 0.0, g[10] ? static_cast<double>(g[9]) / (g[10] * 10.0) : 0.0);
		fprintf(stderr, "[ckl trail diag, k_trail_components, mean cycles per slice] union=%.0f component minima=%.0f starts/splits=%.0f bitmap scan=%.0f\n",
			static_cast<double>(g[12]) / ns, static_cast<double>(g[13]) / ns, static_cast<double>(g[14]) / ns, static_cast<double>(g[15]) / ns);
		fprintf(stderr, "[ckl trail diag, k_trail_segments] waves=%llu iterations/wave mean=%.1f max=%llu cycles/wave mean=%.0f max=%llu cycles/iteration=%.0f active lanes/iteration=%.1f\n",
			g[4], g[4] ? static_cast<double>(g[0]) / g[4] : 0.0, g[1], g[4] ? static_cast<double>(g[2]) / g[4] : 0.0, g[3],
			g[0] ? static_cast<double>(g[2]) / g[0] : 0.0, g[0] ? static_cast<double>(g[5]) / g[0] : 0.0);
	}
	fprintf(stderr, "[ckl trail diag] max degree-1/3/4 vertices of a slice=%u, k_trail_walk LDS=%zu bytes\n", max_special, trail_lds_used);
	fprintf(stderr, "[ckl trail diag, mean per slice] degree-1/3/4 vertices=%.0f corners=%.0f nodes=%.0f starts=%.0f items=%.0f\n", sp, co, m[0], m[3], m[4]);
}

// a slice whose walk ran out of its scratch arrays has said so in d_slice_err
void check_walk_errors(ckl_encoder& e, uint32_t ns) {
	const std::vector<uint32_t> errs = download(e.d_slice_err.p, ns, e.stream);
	for (uint32_t zi = 0; zi < ns; zi++) if (errs[zi]) throw Error(CKL_ERR_RUNTIME, "crackle_amd: crack walk scratch overflow on z=" + std::to_string(zi));
}

// Graph -> walk -> finish -> markov -> gather over the session's planes and node counts (graph_pass): capacities,
// tables, launches, tail.
CrackResult crack_pass(ckl_encoder& e, int64_t sx, int64_t sy, int64_t sz, const CrackRequest& rq) {
	hipStream_t s = e.stream;
	const uint32_t ns = static_cast<uint32_t>(sz);
	const uint64_t nverts = static_cast<uint64_t>(sx + 1) * (sy + 1);
	const int markov_order = rq.markov_order;
	const bool reuse_trail = rq.reuse_trail;
	if (rq.goal == CrackGoal::HISTOGRAM && (!markov_order || rq.model)) throw Error(CKL_ERR_RUNTIME, "crackle_amd: internal: a markov histogram needs an order and no model");
	CrackResult result;
	e.d_slice_err.ensure(ns);
	const bool prezeroed = e.trail_zeroed && !reuse_trail;
	e.trail_zeroed = false;
	if (prezeroed) CKL_HIP(hipStreamWaitEvent(s, e.ev_prezero, 0));
	if (!reuse_trail && !prezeroed) CKL_HIP(hipMemsetAsync(e.d_slice_err.p, 0, ns * sizeof(uint32_t), s));

	// ---- capacities from the exact edge counts (codes <= 7 E, chains <= E, stack <= E)
	std::vector<uint64_t> cbase(ns), sbase(ns), kbase(ns);
	std::vector<uint32_t> ccap(ns), scap(ns), kcap(ns), max_steps(ns);
	std::vector<uint64_t> nbase(ns), cobase(ns), ibase(ns);
	std::vector<uint32_t> ncap(ns), cocap(ns), icap(ns);
	uint64_t ctot = 0, stot = 0, ktot = 0, ntot = 0, cotot = 0, itot = 0;
	uint32_t max_ncap = 0, max_cocap = 0, max_icap = 0, max_special = 0, max_kcap = 0;
	uint64_t max_edges = 0;
	bool any = false;
	for (uint32_t zi = 0; zi < ns; zi++) {
		const uint64_t E = crack_edges(e, sx, sy, zi, rq.permissible);
		any = any || E > 0;
		const uint64_t cc = ((7 * E + 16 + 15) / 16) * 16;      // a multiple of 16: every slice's code arrays start 16-byte aligned (k_finish loads 16 codes at once)
		if (cc > 0xFFFFFFF0ull) throw Error(CKL_ERR_RUNTIME, "crackle_amd: slice has too many crack edges");
		cbase[zi] = ctot; ccap[zi] = static_cast<uint32_t>(cc); ctot += cc;
		max_steps[zi] = static_cast<uint32_t>(E + 1);
		// trail graph: nodes = vertices of degree 1, 3, 4 plus at most one per "right+down" corner
		// (loop starts, chain starts inside a segment); segments <= 2 nodes; items <= 3 segments + 1 per chain
		const uint64_t nc = ((static_cast<uint64_t>(e.count_special[zi]) + e.count_corner[zi] + 16) / 16) * 16;
		if (nc >= (1ull << 28)) throw Error(CKL_ERR_RUNTIME, "crackle_amd: slice has too many crack vertices");
		nbase[zi] = ntot; ncap[zi] = static_cast<uint32_t>(nc); ntot += nc;
		cobase[zi] = cotot; cocap[zi] = e.count_corner[zi]; cotot += e.count_corner[zi];
		const uint64_t ic = 7 * nc + 16;
		ibase[zi] = itot; icap[zi] = static_cast<uint32_t>(ic); itot += ic;
		sbase[zi] = stot; scap[zi] = static_cast<uint32_t>(2 * nc + 4); stot += 2 * nc + 4;
		kbase[zi] = ktot; kcap[zi] = static_cast<uint32_t>(nc); ktot += nc;
		max_ncap = std::max<uint32_t>(max_ncap, ncap[zi]);
		max_cocap = std::max<uint32_t>(max_cocap, cocap[zi]);
		max_icap = std::max<uint32_t>(max_icap, icap[zi]);
		max_special = std::max<uint32_t>(max_special, e.count_special[zi]);
		max_kcap = std::max<uint32_t>(max_kcap, kcap[zi]);
		max_edges = std::max<uint64_t>(max_edges, E);
	}
	result.any_chain = any;
	if (g_ht && g_ht->on) {
		uint32_t over = 0;
		for (uint32_t zi = 0; zi < ns; zi++) over += e.count_special[zi] > 3584u;
		fprintf(stderr, "[ckl trail nodes] max special %u, slices above 3584: %u of %u\n", max_special, over, ns);
	}
	HT_MARK("c:caps");

	// ---- tables: one packed upload; the arrays and output buffers sized from the capacities (no round trip to
	// the host before k_finish)
	UploadPacker tables;
	tables.add(e.d_cbase, cbase); tables.add(e.d_ccap, ccap);
	tables.add(e.d_sbase, sbase); tables.add(e.d_scap, scap);
	tables.add(e.d_kbase, kbase); tables.add(e.d_kcap, kcap);
	// one volume takes one path behind k_trail_items: k_trail_emit, or k_trail_offsets + k_trail_expand + k_finish with a
	// byte per code point in d_cp and d_fcode
	int max_lds = 0;
	CKL_HIP(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, e.device));
	EmitPlan emit;
	if (!reuse_trail) {
		emit = emit_plan(max_edges, max_kcap, max_lds);
		e.emit_fused = emit.fused; e.emit_lds = emit.need;
		if (!emit.fused) { e.d_cp.ensure(ctot); e.d_fcode.ensure(ctot); e.d_chain_clen.ensure(ktot); e.d_chain_vstart.ensure(ktot); }
	}
	if (markov_order) e.d_dcode.ensure(ctot);
	e.d_stack_node.ensure(stot); e.d_stack_code.ensure(stot);
	e.d_chain_node.ensure(ktot); e.d_chain_off.ensure(ktot);
	e.d_chain_order.ensure(ktot); e.d_chain_dst.ensure(ktot);
	e.d_n_chains.ensure(ns); e.d_n_raw.ensure(ns); e.d_n_valid.ensure(ns);
	e.d_payload_len.ensure(ns); e.d_boc_len.ensure(ns);
	const int xw = byte_width(static_cast<uint64_t>(sx) + 1), yw = byte_width(static_cast<uint64_t>(sy) + 1);
	std::vector<uint64_t> pbase(ns), bbase(ns);
	uint64_t ptot = 0, btot = 0;
	for (uint32_t zi = 0; zi < ns; zi++) {
		// codes <= E + 2 (b + t) <= 5 E + 2; plain: 2 bits / code; markov: at most 3 bits / code (+2)
		const uint64_t ncodes = ccap[zi];
		const uint64_t pbytes = markov_order ? (3ull * ncodes + 2 + 7) / 8 : (ncodes + 3) / 4;
		pbase[zi] = ptot; ptot += ((pbytes + 8 + 3) / 4) * 4;
		const uint64_t bbytes = 4 + yw + static_cast<uint64_t>(kcap[zi]) * (yw + 2 * xw);
		bbase[zi] = btot; btot += bbytes;
	}
	tables.add(e.d_pbase, pbase); tables.add(e.d_bbase, bbase);
	tables.add(e.t_nbase, nbase); tables.add(e.t_ncap, ncap);
	tables.add(e.t_cobase, cobase); tables.add(e.t_cocap, cocap);
	tables.add(e.t_ibase, ibase); tables.add(e.t_icap, icap);
	tables.add(e.t_max_steps, max_steps);
	tables.commit(e.d_crack_tables, s, e.uploads_by_kernel ? &e.tables_staging : nullptr);
	HT_MARK("c:tables");
	e.d_payload.ensure(ptot + 8); e.d_boc.ensure(btot + 8);
	e.codes_capacity = ptot + btot;
	if (markov_order) CKL_HIP(hipMemsetAsync(e.d_payload.p, 0, ptot + 8, s));

	// ---- launches: the trail over the node graph (ckl_trail.hpp), unless an earlier pass left it
	DevBuf<unsigned long long> d_tdbg;
	size_t trail_lds_used = 0;
	if (!reuse_trail) {
		e.t_counters.ensure(7 * static_cast<size_t>(ns));
		if (!prezeroed) CKL_HIP(hipMemsetAsync(e.t_counters.p, 0, 7 * static_cast<size_t>(ns) * sizeof(uint32_t), s));
		e.t_node_vertex.ensure(ntot); e.t_node_adj.ensure(ntot + 16); e.t_vert2node.ensure(nverts * ns);
		e.t_corner_vertex.ensure(cotot);
		e.t_dart_end.ensure(4 * ntot); e.t_dart_len.ensure(4 * ntot); e.t_dart_minv.ensure(4 * ntot); e.t_dart_minpos.ensure(4 * ntot);
		e.t_dart_codes.ensure(4 * ntot); e.t_dart_inline.ensure(4 * ntot);
		e.t_parent.ensure(ntot); e.t_compmin.ensure(ntot); e.t_starts.ensure(ntot);
		const uint32_t start_words = static_cast<uint32_t>((nverts + 31) / 32);
		e.t_start_bits.ensure(static_cast<size_t>(start_words) * ns);
		if (!prezeroed) CKL_HIP(hipMemsetAsync(e.t_start_bits.p, 0, static_cast<size_t>(start_words) * ns * sizeof(uint32_t), s));
		e.t_items.ensure(itot); e.t_item_off.ensure(itot); e.t_chain_item0.ensure(ktot);
		e.t_events.ensure(itot); e.t_chain_ev0.ensure(ktot); e.t_ev_lnd.ensure(itot); e.t_ev_item.ensure(itot);
		e.last_trail_slices = ns;

		TrailArgs ta = trail_args(e, sx, sy, ns);
		const FinishArgs fa = finish_args(e, sx, sy, markov_order);
		if (kTuning && getenv("CKL_TRAIL_DIAG")) { d_tdbg.ensure(16); CKL_HIP(hipMemsetAsync(d_tdbg.p, 0, 128, s)); ta.dbg = d_tdbg.p; }
		const size_t budget = static_cast<size_t>(max_lds > 1024 ? max_lds - 1024 : 0);
		const uint32_t dart_blocks = (4 * max_ncap + kWalkChunk * kWaves - 1) / (kWalkChunk * kWaves);
		// union-find table (4 bytes per node) and component minima (8) of k_trail_components in LDS
		size_t clds = (static_cast<size_t>(max_special) + 1024) * 12;
		if (const char* env = getenv("CKL_TRAIL_LDS")) clds = static_cast<size_t>(std::max(0, atoi(env)));
		clds = (std::min(budget, std::max<size_t>(clds, 1024)) / 16) * 16;
		allow_dynamic_lds(reinterpret_cast<const void*>(&k_trail_components), e.device, clds);
		// node tables of k_trail_walk in LDS + 16 KiB of branch stack when that fits
		size_t lds = trail_walk_lds(max_special);      // k_trail_walk: 12 bytes of record + 4 of branch stack per node
		if (const char* env = getenv("CKL_TRAIL_LDS")) lds = static_cast<size_t>(std::max(0, atoi(env)));   // testing: small values force the global tables
		lds = std::min(budget, std::max<size_t>(lds, 4096));
		lds = (lds / 16) * 16;
		allow_dynamic_lds(reinterpret_cast<const void*>(&k_trail_walk), e.device, lds);
		trail_lds_used = lds;
		HT_MARK("c:setup");

		// (Slice groups on streams of their own, so that one group's parallel stages run beside another's serial
		// k_trail_walk, measured at C2: 2 groups between -0.17 and +0.1 ms from run to run, 4 and 8 slower — the
		// DFS wavefronts want their SIMDs to themselves.)
		if (any) {
			hipLaunchKernelGGL(k_trail_nodes, dim3(e.graph_blocks, ns), dim3(kBlock), 0, s, ta);
			hipLaunchKernelGGL(k_trail_segments, dim3(dart_blocks, ns), dim3(kBlock), 0, s, ta);
			if (max_cocap) hipLaunchKernelGGL(k_trail_loops, dim3((max_cocap + kBlock - 1) / kBlock, ns), dim3(kBlock), 0, s, ta);
			hipLaunchKernelGGL(k_trail_components, dim3(ns), dim3(kCompBlock), clds, s, ta, static_cast<uint32_t>(clds));
		}
		CKL_HIP(hipEventRecord(e.evd0, s));
		hipLaunchKernelGGL(k_trail_walk, dim3(ns), dim3(kWave), lds, s, ta, static_cast<uint32_t>(lds));
		CKL_HIP(hipEventRecord(e.evd1, s));
		hipLaunchKernelGGL(k_trail_items, dim3(ns), dim3(kItemsBlock), 0, s, ta);
		if (emit.fused) {
			allow_dynamic_lds(reinterpret_cast<const void*>(&k_trail_emit), e.device, emit.dyn);
			hipLaunchKernelGGL(k_trail_emit, dim3(ns), dim3(kEmitBlock), emit.dyn, s, ta, fa, emit.tcap, emit.wcap);
		}
		else {
			hipLaunchKernelGGL(k_trail_offsets, dim3(ns), dim3(kBlock), 0, s, ta);
			hipLaunchKernelGGL(k_trail_expand, dim3((max_icap + kExpandChunk * kWaves - 1) / (kExpandChunk * kWaves), ns), dim3(kBlock), 0, s, ta);
			hipLaunchKernelGGL(k_finish, dim3(ns), dim3(kFinishBlock), 0, s, fa);
		}
	}
	HT_MARK("c:enqueue");
	if (kTuning && getenv("CKL_TRAIL_DIAG")) trail_diag(e, ns, d_tdbg.p, max_special, trail_lds_used);

	// ---- tail.  Without a markov model nothing stands between k_finish and the final offsets + gather: they are
	// enqueued before the label side takes the host thread (it is host-synchronous and ends after the trail: the
	// trail's queue used to idle 0.2 ms until the host came back to launch them)
	auto enqueue_tail = [&]() {
		e.d_out_off.ensure(ns);
		e.d_code_report.ensure(static_cast<size_t>(ns) + 3);
		e.d_codes_out.ensure(e.codes_capacity + 8);
		hipLaunchKernelGGL(k_code_offsets, dim3(1), dim3(kBlock), 0, s, e.d_boc_len.p, e.d_payload_len.p, e.d_slice_err.p, ns, e.d_out_off.p, e.d_code_report.p);
		hipLaunchKernelGGL(k_gather_codes, dim3(ns), dim3(kBlock), 0, s, e.d_boc.p, e.d_bbase.p, e.d_boc_len.p,
			e.d_payload.p, e.d_pbase.p, e.d_payload_len.p, e.d_out_off.p, e.d_codes_out.p);
	};
	if (!markov_order) enqueue_tail();
	// the label side (other stream, host-synchronous) runs while the trail kernels execute
	if (rq.overlap) rq.overlap();
	HT_MARK("c:overlap");

	if (markov_order) {
		if (rq.model) result.model = *rq.model;
		else {
			const size_t rows = static_cast<size_t>(1) << (2 * markov_order);
			e.d_hist.ensure(rows * 4);
			CKL_HIP(hipMemsetAsync(e.d_hist.p, 0, rows * 4 * sizeof(uint32_t), s));
			const uint32_t hist_lds = (rows * 4 <= 16384) ? static_cast<uint32_t>(rows * 4) : 0u;    // order <= 6: 64 KiB
			allow_dynamic_lds(reinterpret_cast<const void*>(&k_markov_hist), e.device, hist_lds * 4);
			hipLaunchKernelGGL(k_markov_hist, dim3(ns), dim3(kBlock), hist_lds * sizeof(uint32_t), s, e.d_dcode.p, e.d_cbase.p, e.d_n_valid.p, markov_order, e.d_hist.p, hist_lds);
			result.hist = download(e.d_hist.p, rows * 4, s);
			if (rq.goal == CrackGoal::HISTOGRAM) { check_walk_errors(e, ns); return result; }
			result.model = markov_stats_to_model(result.hist.data(), rows);
		}
		upload(e.d_model, result.model, s);
		hipLaunchKernelGGL(k_markov_pack, dim3(ns), dim3(kBlock), 0, s, e.d_dcode.p, e.d_cbase.p, e.d_n_valid.p, markov_order,
			e.d_model.p, e.d_pbase.p, e.d_payload.p, e.d_payload_len.p);
		// final offsets on the device, the gather behind them
		enqueue_tail();
	}
	// one small report back (lengths for the z-index, total, error bits): a single wait before the codes are copied out
	HT_MARK("c:finish_enq");
	const std::vector<uint32_t> report = download(e.d_code_report.p, static_cast<size_t>(ns) + 3, s);
	HT_MARK("c:finish_wait");
	if (report[ns + 2]) check_walk_errors(e, ns);
	result.code_len.assign(report.begin(), report.begin() + ns);
	result.total = static_cast<uint64_t>(report[ns]) | (static_cast<uint64_t>(report[ns + 1]) << 32);
	return result;
}

}  // namespace

// The stream's header as the volume's statistics decide it (crackle.hpp:50-64, 233-235) unless the overrides do;
// of an empty volume (all statistics 0) it is the whole stream (crackle.hpp:96-98).  num_label_bytes comes later.
Header ckl::stream_header(int data_width, int64_t sx, int64_t sy, int64_t sz, const VolumeStats& st, bool allow_pins, bool fortran_order, uint64_t markov_model_order, const ckl_encode_overrides* ov) {
	Header head;
	head.crack_format = IMPERMISSIBLE;
	head.label_format = PINS_VARIABLE_WIDTH;
	if (static_cast<int64_t>(st.pairs) < static_cast<int64_t>(static_cast<uint64_t>(sx) * sy * sz) / 2) {   // crackle.hpp:50-55
		head.crack_format = PERMISSIBLE;
		head.label_format = FLAT;
	}
	if (ov && ov->force_crack_format >= 0) {
		head.crack_format = ov->force_crack_format;
		head.label_format = ov->force_crack_format == PERMISSIBLE ? FLAT : PINS_VARIABLE_WIDTH;
	}
	if (sz == 1 || !allow_pins) head.label_format = FLAT;           // crackle.hpp:62-64
	if (ov && ov->force_label_format >= 0) head.label_format = ov->force_label_format;
	head.is_signed = false;
	head.data_width = data_width;
	head.stored_data_width = ov && ov->force_stored_width ? ov->force_stored_width : byte_width(st.max_label);      // crackle.hpp:233-235
	head.sx = static_cast<uint32_t>(sx); head.sy = static_cast<uint32_t>(sy); head.sz = static_cast<uint32_t>(sz);
	head.log2_grid_size = 31;
	head.fortran_order = fortran_order;
	head.markov_model_order = static_cast<int>(markov_model_order & 0xFF);
	head.is_sorted = true;
	return head;
}

void ckl::check_dims(int64_t sx, int64_t sy, int64_t sz, int dtype_bytes, int is_signed) {
	if (is_signed) throw Error(CKL_ERR_ARG, "Signed integer data types are not currently supported.");
	if (dtype_bytes != 1 && dtype_bytes != 2 && dtype_bytes != 4 && dtype_bytes != 8) throw Error(CKL_ERR_ARG, "crackle_amd: dtype width must be 1, 2, 4 or 8 bytes");
	if (sx < 0 || sy < 0 || sz < 0) throw Error(CKL_ERR_ARG, "crackle_amd: negative dimension");
	if (sx > 0x7FFFFFF0ll || sy > 0x7FFFFFF0ll || sz > 0x7FFFFFF0ll) throw Error(CKL_ERR_ARG, "crackle_amd: dimension too large");
	// (slices of 2^30 or more pixels encode into streams this decoder refuses, and one such encode faulted on the
	// device: until the 32-bit arithmetic behind that is found, the limit is 2^30 crack vertices)
	if (static_cast<uint64_t>(sx + 1) * static_cast<uint64_t>(sy + 1) >= (1ull << 30)) throw Error(CKL_ERR_ARG, "crackle_amd: slices of 2^30 or more crack vertices are not supported");
}

void ckl::planes_adopt(ckl_encoder& e, uint32_t row_words, uint64_t plane_words, uint32_t ns, uint32_t count_rows) {
	e.row_words = row_words;
	e.plane_words = plane_words;
	e.d_planes.ensure(2 * plane_words * ns);
	e.d_count_vh.ensure(4 * static_cast<size_t>(ns));
	CKL_HIP(hipMemsetAsync(e.d_count_vh.p, 0, count_rows * static_cast<size_t>(ns) * sizeof(uint32_t), e.stream));
}

void ckl::planes_adopt_counts(ckl_encoder& e, const std::vector<uint32_t>& counts, uint32_t ns) {
	e.count_v.assign(counts.begin(), counts.begin() + ns);
	e.count_h.assign(counts.begin() + ns, counts.begin() + 2 * static_cast<size_t>(ns));
}

namespace {

// what a run makes of its volume: ckl_encoder_run's arguments (include/crackle_amd.h)
struct EncodeRequest {
	bool allow_pins = false, fortran_order = false;
	uint64_t markov_model_order = 0;
	bool optimize_pins = false, auto_bgcolor = true;
	int64_t manual_bgcolor = 0;
	const ckl_encode_overrides* overrides = nullptr;
};

// When does the label stream's component labelling run?  Beside the trail's chip-filling kernels the two
// take turns (graph 0.2 -> 0.65 ms at C2); the serial walk leaves the chip idle for a millisecond, and
// two walks per CU leave room for other workgroups when they keep to a third of the LDS each.  Then the
// label stream starts with the walk (it waits for the event in front of it): AT_WALK.  Otherwise it starts
// in front of the graph kernel, BEFORE_GRAPH: slices too large for that (decided from their size, before the node
// counts are known), CKL_NO_OVERLAP, CKL_LABELS_AT_WALK=0; or behind it, AFTER_GRAPH, when the node counts say that the
// walks leave no room.  (The sharded encode's label stream also carries the ranks' exchange of unique
// labels: 0.5 ms on the host.  It fits since the slab's labels are exchanged unsorted.)
enum class LabelStart { BEFORE_GRAPH, AFTER_GRAPH, AT_WALK };

// The one place that decides it.  Asked twice: before the planes pass, without the graph's node counts, the answer is
// BEFORE_GRAPH or "not before" (AFTER_GRAPH); with them (e.count_special of graph_pass) it is final.
LabelStart label_start(const ckl_encoder& e, int64_t sx, int64_t sy, bool no_overlap, const std::vector<uint32_t>* count_special = nullptr) {
	const char* at_walk = getenv("CKL_LABELS_AT_WALK");
	if (no_overlap || static_cast<uint64_t>(sx) * sy > (1536ull * 1536ull) || (at_walk && atoi(at_walk) == 0)) return LabelStart::BEFORE_GRAPH;
	if (!count_special) return LabelStart::AFTER_GRAPH;
	uint32_t max_special = 0;
	for (uint32_t v : *count_special) max_special = std::max(max_special, v);
	int max_lds = 0;
	CKL_HIP(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, e.device));
	const bool beside_walks = max_special < 5000 && 2 * trail_walk_lds(max_special) + kFlatResolveLds <= static_cast<size_t>(max_lds);
	return beside_walks ? LabelStart::AT_WALK : LabelStart::AFTER_GRAPH;
}

// What the early output buffer (label_stage) allows for behind the label section: the stored model and the
// crack code bytes, estimated from the edge and node counts: every edge is one code, a branch
// costs a few more; 2 bits per code (markov: at most 3), BOC index of a few chains per slice
uint64_t estimate_code_bytes(const ckl_encoder& e, int64_t sx, int64_t sy, int64_t sz, bool permissible, int markov_order) {
	uint64_t est_code_bytes = 0;
	const int xw = byte_width(static_cast<uint64_t>(sx) + 1), yw = byte_width(static_cast<uint64_t>(sy) + 1);
	for (int64_t z = 0; z < sz; z++) {
		const uint64_t codes = crack_edges(e, sx, sy, z, permissible) + 4ull * (static_cast<uint64_t>(e.count_special[z]) + e.count_corner[z]) + 16;
		est_code_bytes += (markov_order ? (3 * codes + 7) / 8 : (codes + 3) / 4) + 8;
		est_code_bytes += 4 + yw + 64ull * (yw + 2 * xw);
	}
	if (getenv("CKL_SMALL_ESTIMATE")) est_code_bytes = 0;      // testing: the stream outgrows the early buffer
	const uint64_t model_bytes_est = markov_order ? (1ull << (2 * markov_order)) : 0;
	return model_bytes_est + est_code_bytes;
}

// where the label section begins: behind the header and the z-index
inline uint64_t labels_offset(const Header& head) { return head.header_bytes() + head.grid_index_bytes(); }

// what the label side of a run leaves for the assembly
struct LabelSide {
	FlatResult flat;                       // per slice: the components and the crc of the component image
	uint64_t label_bytes = 0;
	std::vector<uint8_t> pins_binary;      // pin label section (host built)
	uint32_t labels_crc = 0;               // of the flat label section, unless labels_stay
	bool labels_stay = false;              // the label section and its crc stay on the device until the background copy
	HostOut<uint8_t> early;                // flat labels: the output buffer, taken early, with the label section in it unless labels_stay
	uint64_t early_cap = 0;
};

// The label side (labels.hpp:30-155): runs on the host while the trail kernels execute (CrackRequest::overlap).  The
// components + crcs that were started on the label stream are collected here, or started here when they start with the
// walk; then the label section.  behind_labels: estimate_code_bytes.
template <typename LABEL>
LabelSide label_stage(
	ckl_encoder& e, const LABEL* labels, int64_t sx, int64_t sy, int64_t sz, const Header& head, const EncodeRequest& req, LabelStart start, uint64_t behind_labels
) {
	LabelSide r;
	hipStream_t s2 = e.stream2;
	if (start == LabelStart::AT_WALK) {
		CKL_HIP(hipStreamWaitEvent(s2, e.evd0, 0));      // (starting one kernel earlier, beside k_trail_components, cost 0.2 ms)
		flat_enqueue(e, labels, sx, sy, sz, head.label_format != FLAT, true);
	}
	flat_collect(e, labels, static_cast<int>(sizeof(LABEL)), sx, sy, sz, r.flat);
	HT_MARK("flat");
	const uint64_t N = r.flat.total;
	if (head.label_format == PINS_VARIABLE_WIDTH) {
		// pins (pins.hpp:348-403, labels.hpp:157-344): components and crcs come from the
		// device passes above; the order-sensitive cover runs on the host (ckl_pins.hip)
		if (N > 0xFFFFFFFFull) throw Error(CKL_ERR_RUNTIME, "crackle_amd: too many components");
		e.d_cc_volume.ensure(static_cast<uint64_t>(sx) * sy * sz);
		paint_components(e, sx, sy, sz, 0u, e.d_cc_volume.p);
		r.pins_binary = pins_section_plain<LABEL>(e, labels, e.d_cc_volume.p, e.d_mapping.p, sx, sy, sz, N, r.flat.ncomp, head.pin_index_width(), head.stored_data_width, req.auto_bgcolor, req.manual_bgcolor);
		r.label_bytes = r.pins_binary.size();
		return r;
	}
	const uint64_t off_labels = labels_offset(head);
	r.label_bytes = flat_section(e, N, head.stored_data_width, byte_width(static_cast<uint64_t>(sx) * sy), static_cast<uint32_t>(sz), req.overrides);
	HT_MARK("label_table");
	r.labels_stay = e.async_host_copy && e.keep_device_stream && !e.defer_codes && r.label_bytes > 0;
	// The output buffer is taken now, sized with an estimate of the crack code bytes, so that
	// the label section is copied out and checksummed while the trail still runs; a stream
	// that outgrows the estimate is moved to a larger buffer at assembly.
	r.early_cap = off_labels + r.label_bytes + behind_labels + 4ull * (sz + 1) + 64;
	r.early = host_out<uint8_t>(r.early_cap);
	HT_MARK("l:buffer");
	uint8_t* eo = r.early.get();
	// (one copy: four pieces with an event each, checksummed while the next was on the link, saved 0.04 ms
	// and now and then stalled the enqueueing thread for milliseconds)
	if (r.labels_stay) {
		// the caller goes on from the stream in HBM: the section's crc32c is taken on the device and the section itself travels
		// to the host with the crack codes, in the background (until round 5 both sat on the encode's tail: 8 MB over the link,
		// then the host's crc over them, 0.25 ms at C2)
		e.d_labels_crc.ensure(1 + kBlock);
		if (!e.ev_labels_crc) CKL_HIP(hipEventCreateWithFlags(&e.ev_labels_crc, hipEventDisableTiming));
		crc32c_device(e.d_labels_bin.p, r.label_bytes, e.d_labels_crc.p + 1, e.d_labels_crc.p, s2);
		CKL_HIP(hipEventRecord(e.ev_labels_crc, s2));
	}
	else {
		if (r.label_bytes) CKL_HIP(hipMemcpyAsync(eo + off_labels, e.d_labels_bin.p, r.label_bytes, hipMemcpyDeviceToHost, s2));
		CKL_HIP(hipStreamSynchronize(s2));
		r.labels_crc = crc32c(eo + off_labels, r.label_bytes);
	}
	HT_MARK("labels_d2h");
	return r;
}

// Where a stream's sections lie (crackle.hpp:171-216):
//   header | z-index + crc | labels | model | crack codes | labels crc | slice crcs
// A version 0 stream, which only reencode_markov writes, has a 24-byte header, no crc behind the z-index and no tail.
struct StreamLayout { uint64_t off_index, off_labels, off_model, off_codes, off_tail, total; };
StreamLayout stream_layout(const Header& head, uint64_t model_bytes, uint64_t code_bytes) {
	StreamLayout l;
	l.off_index = head.header_bytes();
	l.off_labels = labels_offset(head);
	l.off_model = l.off_labels + head.num_label_bytes;
	l.off_codes = l.off_model + model_bytes;
	l.off_tail = l.off_codes + code_bytes;
	l.total = l.off_tail + (head.format_version == 0 ? 0 : 4ull * (static_cast<uint64_t>(head.sz) + 1));
	return l;
}

inline void put4(uint8_t* p, uint32_t v) { for (int b = 0; b < 4; b++) p[b] = static_cast<uint8_t>((v >> (8 * b)) & 0xFF); }

// what frames the sections that are copied or computed elsewhere: the header, the z-index (every slice's code bytes) with its
// crc, and the stored model
void write_frame(uint8_t* o, const Header& head, const StreamLayout& l, const std::vector<uint32_t>& code_len, const std::vector<uint8_t>& stored_model) {
	std::vector<uint8_t> hb;
	head.write(hb);
	memcpy(o, hb.data(), hb.size());
	const uint64_t sz = head.sz;
	for (uint64_t z = 0; z < sz; z++) put4(o + l.off_index + 4 * z, code_len[z]);
	if (head.format_version != 0) put4(o + l.off_index + 4 * sz, crc32c(o + l.off_index, 4 * sz));
	if (!stored_model.empty()) memcpy(o + l.off_model, stored_model.data(), stored_model.size());
}

// The bulky sections reach the stream `o`, whose frame, flat label section (unless labels_stay) and tail the host has
// written: the stream once more in HBM if the session keeps one, then the crack codes' way to the host.
void assemble(ckl_encoder& e, uint8_t* o, const Header& head, const StreamLayout& l, bool labels_stay) {
	hipStream_t s = e.stream;
	const uint64_t label_bytes = head.num_label_bytes, model_bytes = l.off_codes - l.off_model, code_bytes = l.off_tail - l.off_codes;
	e.device_stream_bytes = 0;
	if (e.keep_device_stream) {
		// the same bytes once more in HBM, for a decoder that takes its stream from the device
		// (ckl_decoder_create_device): the two bulky sections are device-to-device copies, the small
		// ones go up from the host buffer
		e.d_stream_out.ensure(l.total + 16);
		uint8_t* ds = e.d_stream_out.p;
		const void* up = head.label_format == FLAT ? o : nullptr;      // (by kernel for flat label streams only, see upload_small; o: a pinned, device-mapped block when the stream is 64 KiB or more)
		upload_small(ds, o, l.off_labels, s, up);
		if (label_bytes) {
			if (head.label_format == FLAT) copy_bytes_device(e.d_labels_bin.p, ds + l.off_labels, label_bytes, s);
			else CKL_HIP(hipMemcpyAsync(ds + l.off_labels, o + l.off_labels, label_bytes, hipMemcpyHostToDevice, s));
		}
		if (model_bytes) upload_small(ds + l.off_model, o + l.off_model, model_bytes, s, up);
		if (code_bytes) copy_bytes_device(e.d_codes_out.p, ds + l.off_codes, code_bytes, s);
		upload_small(ds + l.off_tail, o + l.off_tail, l.total - l.off_tail, s, up);
		if (labels_stay) {
			CKL_HIP(hipStreamWaitEvent(s, e.ev_labels_crc, 0));
			CKL_HIP(hipMemcpyAsync(ds + l.off_tail, e.d_labels_crc.p, 4, hipMemcpyDeviceToDevice, s));
		}
		e.device_stream_bytes = l.total;
	}
	// the crack codes' copy to the host goes LAST: started first, its 13 MB kept the link busy and the 2 KB header
	// upload above waited 0.19 ms behind it (rocprofv3 timeline, round 4)
	if (code_bytes && !e.defer_codes) {
		if (e.async_host_copy && e.keep_device_stream) {
			// the caller goes on with the stream in HBM (a decoder, the next volume's planes) while the codes
			// cross PCIe: ckl_encoder_host_wait before the host bytes are read
			if (!e.stream_copy) CKL_HIP(hipStreamCreateWithFlags(&e.stream_copy, hipStreamNonBlocking));
			if (!e.ev_codes) CKL_HIP(hipEventCreateWithFlags(&e.ev_codes, hipEventDisableTiming));
			CKL_HIP(hipEventRecord(e.ev_codes, s));
			CKL_HIP(hipStreamWaitEvent(e.stream_copy, e.ev_codes, 0));
			CKL_HIP(hipMemcpyAsync(o + l.off_codes, e.d_codes_out.p, code_bytes, hipMemcpyDeviceToHost, e.stream_copy));
			if (labels_stay) {
				CKL_HIP(hipMemcpyAsync(o + l.off_labels, e.d_labels_bin.p, label_bytes, hipMemcpyDeviceToHost, e.stream_copy));
				CKL_HIP(hipMemcpyAsync(o + l.off_tail, e.d_labels_crc.p, 4, hipMemcpyDeviceToHost, e.stream_copy));
			}
			e.host_copy_pending = true;
		}
		else CKL_HIP(hipMemcpyAsync(o + l.off_codes, e.d_codes_out.p, code_bytes, hipMemcpyDeviceToHost, s));
	}
}

// One run, in the order of its steps (DESIGN.md §8 states the schedule): planes, graph, the label stream's start at one of
// three places (label_start), the crack trail with the label side under it, the frame, the assembly.
template <typename LABEL>
void encode_typed(ckl_encoder& e, const LABEL* labels, int64_t sx, int64_t sy, int64_t sz, const EncodeRequest& req, uint8_t** out, uint64_t* out_len) {
	const ckl_encode_overrides* const ov = req.overrides;
	const uint64_t voxels = static_cast<uint64_t>(sx) * sy * sz;
	hipStream_t s = e.stream;
	CKL_HIP(hipEventRecord(e.ev0, s));

	HostTimer ht;
	g_ht = &ht;
	VolumeStats st;
	e.trail_zeroed = false;
	// (recompress: the planes were built from a decode session's run tables, there is no volume)
	const bool have_planes = voxels > 0 && (e.label_src ? planes_cached(e, e.label_src, sx, sy, sz) : ov && planes_cached(e, labels, sx, sy, sz));
	e.planes_for = nullptr;       // single use: the caller may change the volume afterwards
	if (e.label_src && voxels > 0 && !have_planes) throw Error(CKL_ERR_RUNTIME, "crackle_amd: internal: recompress without its planes");
	const bool no_overlap = getenv("CKL_NO_OVERLAP") != nullptr;      // diagnostic: kernel timings without the two streams competing
	LabelStart start = label_start(e, sx, sy, no_overlap);
	// (a label stream that starts in front of the graph kernel sizes its run arrays from the planes' counts: no deferral then)
	if (voxels > 0 && !have_planes) planes_pass<LABEL>(e, labels, sx, sy, sz, &st, start != LabelStart::BEFORE_GRAPH);
	else if (have_planes) st = e.planes_stats;      // overrides that force nothing still decide from the volume
	ht.mark("planes");
	bool graph_done = false;
	if (e.planes_deferred) {
		// the planes kernel's counts are still on the device: the graph kernel goes behind it without a round
		// trip (it reads the crack format's deciding pair count there), both kernels' counts come in one
		e.trail_for = nullptr;
		graph_pass(e, sx, sy, sz, ov && ov->force_crack_format >= 0 ? graph_format(ov->force_crack_format == PERMISSIBLE) : GraphFormat::ON_DEVICE, &st);
		graph_done = true;
		ht.mark("graph");
	}
	Header head = stream_header(static_cast<int>(sizeof(LABEL)), sx, sy, sz, st, req.allow_pins, req.fortran_order, req.markov_model_order, ov);
	e.uploads_by_kernel = head.label_format == FLAT;
	if (voxels == 0) { hand_out(header_bytes(head), OutAlloc::MALLOC, out, out_len); return; }
	if (req.optimize_pins) throw Error(CKL_ERR_ARG, "crackle_amd: allow_pins=2 (find_optimal_pins) is out of scope");
	if (head.label_format != FLAT && head.label_format != PINS_VARIABLE_WIDTH) throw Error(CKL_ERR_ARG, "crackle_amd: unsupported label format");
	if (head.markov_model_order > 13) throw Error(CKL_ERR_ARG, "crackle_amd: markov_model_order > 13 is not supported on device");

	// labels (labels.hpp:30-155): components + crcs start on the label stream, here, behind the graph kernel or with
	// the walk (label_stage), and are collected while the crack trail runs
	const bool need_runs = head.label_format != FLAT;      // pins paint the component volume from the run tables
	if (start == LabelStart::BEFORE_GRAPH) flat_enqueue(e, labels, sx, sy, sz, need_runs, false);
	const bool trail_cached = !graph_done && have_planes && ov && ov->has_model && head.markov_model_order > 0 && e.trail_for == static_cast<const void*>(labels)
		&& e.trail_perm == (head.crack_format == PERMISSIBLE) && e.trail_order == head.markov_model_order;
	e.trail_for = nullptr;
	if (graph_done && e.graph_permissible != (head.crack_format == PERMISSIBLE)) throw Error(CKL_ERR_RUNTIME, "crackle_amd: internal: device and host disagree on the crack format");
	if (!trail_cached && !graph_done) graph_pass(e, sx, sy, sz, graph_format(head.crack_format == PERMISSIBLE));
	ht.mark("graph");
	start = label_start(e, sx, sy, no_overlap, &e.count_special);
	if (start == LabelStart::AFTER_GRAPH) flat_enqueue(e, labels, sx, sy, sz, need_runs, false);

	const bool permissible = head.crack_format == PERMISSIBLE;
	// if no slice has a crack edge the reference resets the markov order to 0 (crackle.hpp:107-118)
	{
		bool any = false;
		for (int64_t z = 0; z < sz && !any; z++) any = crack_edges(e, sx, sy, z, permissible) > 0;
		if (!any && !(ov && ov->has_model)) head.markov_model_order = 0;
	}
	std::vector<uint8_t> forced_model;
	CrackRequest crq;
	crq.permissible = permissible;
	crq.markov_order = head.markov_model_order;
	crq.reuse_trail = trail_cached;
	if (ov && ov->has_model && head.markov_model_order > 0) {
		const size_t rows = static_cast<size_t>(1) << (2 * head.markov_model_order);
		forced_model.assign(ov->model, ov->model + rows * 4);
		crq.model = &forced_model;
	}

	const uint64_t behind_labels = estimate_code_bytes(e, sx, sy, sz, permissible, head.markov_model_order);
	LabelSide side;
	auto label_side = [&]() { side = label_stage<LABEL>(e, labels, sx, sy, sz, head, req, start, behind_labels); };
	if (!no_overlap) crq.overlap = label_side;
	const CrackResult cr = crack_pass(e, sx, sy, sz, crq);
	if (no_overlap) label_side();
	ht.mark("cracks");
	std::vector<uint8_t> stored_model;
	if (head.markov_model_order > 0) stored_model = markov_model_to_stored(cr.model);

	// assembly (crackle.hpp:171-216), straight into the caller's buffer
	head.num_label_bytes = side.label_bytes;
	const StreamLayout l = stream_layout(head, stored_model.size(), cr.total);
	uint8_t* o;
	if (side.early && l.total <= side.early_cap) o = side.early.release();
	else {
		o = static_cast<uint8_t*>(host_out_alloc(l.total));
		if (side.early && side.label_bytes) memcpy(o + l.off_labels, side.early.get() + l.off_labels, side.label_bytes);
	}
	try {
		e.last_codes_total = cr.total;
		if (head.label_format == PINS_VARIABLE_WIDTH) {
			if (side.label_bytes) memcpy(o + l.off_labels, side.pins_binary.data(), side.label_bytes);
			side.labels_crc = crc32c(o + l.off_labels, side.label_bytes);
		}
		write_frame(o, head, l, cr.code_len, stored_model);
		for (int64_t z = 0; z < sz; z++) put4(o + l.off_tail + 4 + 4ull * z, side.flat.crcs[z]);
		put4(o + l.off_tail, side.labels_crc);
		assemble(e, o, head, l, side.labels_stay);
		ht.mark("assembly");
		CKL_HIP(hipEventRecord(e.ev1, s));
		CKL_HIP(hipStreamSynchronize(s));
		ht.mark("codes_d2h");
		CKL_HIP(hipGetLastError());
		CKL_HIP(hipEventElapsedTime(&e.pipeline_ms, e.ev0, e.ev1));
		CKL_HIP(hipEventElapsedTime(&e.dominant_ms, e.evd0, e.evd1));      // the encoder's longest kernel: k_trail_walk
	}
	catch (...) {
		// the codes' background copy may already be queued into `o`: it must be over before the block goes back to the cache
		drain_host_copy(e, true);
		host_out_free(o);
		throw;
	}
	if (e.label_src) e.host_marks = ht.marks;      // recompress (ckl_recompress.hip) folds them into its own line
	*out = o;
	*out_len = l.total;
}

}  // namespace

// (declared in ckl_encoder.hpp) encode_typed goes on as it does from cached planes, with the label stage reading
// `labels`: the planes, max label and pixel pairs are functions of the labels alone, and everything behind them is the
// encoder's own, so the bytes are those of compress() of the volume the tables describe.
void ckl::encode_from_planes(
	ckl_encoder& e, const RunLabels& labels, int64_t sx, int64_t sy, int64_t sz, int data_width, bool fortran_order,
	uint64_t markov_model_order, const VolumeStats& st, const std::vector<uint32_t>& counts, uint8_t** out, uint64_t* out_len
) {
	planes_adopt_counts(e, counts, static_cast<uint32_t>(sz));
	e.planes_stats = st;
	e.planes_deferred = false;
	e.planes_dims[0] = sx; e.planes_dims[1] = sy; e.planes_dims[2] = sz;
	struct Source {
		ckl_encoder& e;
		Source(ckl_encoder& enc, const RunLabels* l) : e(enc) { e.label_src = l; e.planes_for = l; }
		~Source() { e.label_src = nullptr; e.planes_for = nullptr; }
	} source(e, &labels);
	const EncodeRequest req = { false, fortran_order, markov_model_order };      // (the rest: no pins, the background colour chosen, no overrides)
	with_label_type(data_width, [&](auto t) { encode_typed<typename decltype(t)::type>(e, nullptr, sx, sy, sz, req, out, out_len); });
}

namespace {

// reencode_with_markov_order (src/crackle.hpp:858-984).  The reference takes every slice's
// code apart into symbols and packs them again; here the decoder rasterises the codes into the
// crack planes and the encoder's trail writes them out again under the new order.  The trail is a
// function of the crack set alone, so the code points are the ones the reference's own encoder
// gives for these slices — which is what its reencode reproduces for any stream that encoder
// (or this one) wrote.  Header, z-index and model are rewritten, label section and crcs copied.
void reencode_markov(const uint8_t* buf, uint64_t n, int markov_order, int device, uint8_t** out, uint64_t* out_len) {
	if (n < Header::kBytesV0) throw Error(CKL_ERR_FORMAT, "crackle: Input too small to be a valid stream. Bytes: " + std::to_string(n));
	Header head = Header::parse(buf, n);
	if (markov_order < 0 || markov_order > 13) throw Error(CKL_ERR_ARG, "crackle_amd: markov_model_order must be in [0, 13] on device");
	if (head.markov_model_order == markov_order) { hand_out(buf, n, OutAlloc::HOST_OUT, out, out_len); return; }      // crackle.hpp:887-889
	// Version 0 streams (24-byte header, no crcs) stay version 0, as src/crackle.hpp:947-984 means them to: the
	// reference's own output for them is broken — its header vector has 29 bytes of which 24 are written
	// (src/header.hpp:277-281), so five stray zero bytes follow the header (tests/golden/v0.npz keeps a sample) —
	// what is written here is the stream that code intends, which the reference reads back.
	const bool v0 = head.format_version == 0;
	const uint64_t sz = head.sz;
	const uint64_t tail_bytes = v0 ? 0 : 4 * (sz + 1);
	const uint64_t off_index = head.header_bytes();
	const uint64_t off_labels = off_index + head.grid_index_bytes();
	if (!head.layout_fits(n)) throw Error(CKL_ERR_RUNTIME, "crackle: get_crack_code_offsets: Unable to read past end of buffer.");      // no sum of untrusted fields that could wrap
	const uint64_t old_codes = off_labels + head.num_label_bytes + head.markov_model_bytes();
	uint64_t old_tail = old_codes;
	for (uint64_t z = 0; z < sz; z++) old_tail += rd_le(buf + off_index + 4 * z, 4);
	if (old_tail > n || tail_bytes > n - old_tail) throw Error(CKL_ERR_RUNTIME, "crackle: get_crack_codes: Unable to read past end of buffer.");

	const bool prof = getenv("CKL_PROFILE") != nullptr;
	auto t_prev = std::chrono::steady_clock::now();
	auto lap = [&](const char* what) {
		if (!prof) return;
		const auto now = std::chrono::steady_clock::now();
		fprintf(stderr, "[ckl reencode host ms] %s=%.2f\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
		t_prev = now;
	};
	struct DecoderGuard { ckl_decoder* d = nullptr; ~DecoderGuard() { if (d) ckl_decoder_destroy(d); } } dec;
	struct EncoderGuard { ckl_encoder* e = nullptr; ~EncoderGuard() { if (e) ckl_encoder_destroy(e); } } enc;
	if (ckl_decoder_create(buf, n, 0, -1, device, &dec.d) != CKL_OK) throw Error(CKL_ERR_RUNTIME, ckl_last_error());
	lap("decoder_create");
	CrackResult cr;
	std::vector<uint8_t> stored_model;
	head.markov_model_order = markov_order;
	if (head.voxels() > 0) {
		const uint32_t *cv = nullptr, *ch = nullptr;
		uint32_t row_words = 0;
		uint64_t plane_words = 0;
		if (ckl_decoder_crack_planes(dec.d, &cv, &ch, &row_words, &plane_words) != CKL_OK) throw Error(CKL_ERR_RUNTIME, ckl_last_error());
		lap("crack_planes");
		if (ckl_encoder_create(head.sx, head.sy, head.sz, 1, device, &enc.e) != CKL_OK) throw Error(CKL_ERR_RUNTIME, ckl_last_error());
		lap("encoder_create");
		ckl_encoder& e = *enc.e;
		hipStream_t s = e.stream;
		const uint32_t ns = head.sz;
		const bool permissible = head.crack_format == PERMISSIBLE;
		planes_adopt(e, row_words, plane_words, ns, 2);
		hipLaunchKernelGGL(k_planes_from_cracks, dim3(static_cast<uint32_t>((plane_words + kBlock - 1) / kBlock), ns), dim3(kBlock), 0, s,
			cv, ch, head.sx, head.sy, row_words, plane_words, permissible ? 1u : 0u,
			plane_v(e), plane_h(e, ns), e.d_count_vh.p, ns);
		planes_adopt_counts(e, download(e.d_count_vh.p, 2 * static_cast<size_t>(ns), s), ns);
		lap("planes");
		graph_pass(e, head.sx, head.sy, head.sz, graph_format(permissible));
		lap("graph");
		CrackRequest crq;
		crq.permissible = permissible;
		crq.markov_order = markov_order;
		cr = crack_pass(e, head.sx, head.sy, head.sz, crq);
		lap("cracks");
		if (markov_order > 0) stored_model = markov_model_to_stored(cr.model);
	}
	else cr.code_len.assign(sz, 0);

	// assembly (crackle.hpp:935-981)
	const StreamLayout l = stream_layout(head, stored_model.size(), cr.total);
	uint8_t* o = static_cast<uint8_t*>(host_out_alloc(l.total));
	try {
		if (cr.total) CKL_HIP(hipMemcpyAsync(o + l.off_codes, enc.e->d_codes_out.p, cr.total, hipMemcpyDeviceToHost, enc.e->stream));
		write_frame(o, head, l, cr.code_len, stored_model);
		memcpy(o + l.off_labels, buf + l.off_labels, head.num_label_bytes);
		if (tail_bytes) memcpy(o + l.off_tail, buf + old_tail, tail_bytes);
		if (cr.total) CKL_HIP(hipStreamSynchronize(enc.e->stream));
		lap("assembly");
	}
	catch (...) { host_out_free(o); throw; }
	*out = o;
	*out_len = l.total;
}

}  // namespace

extern "C" {

int ckl_encoder_create(int64_t sx, int64_t sy, int64_t sz, int dtype_bytes, int device, ckl_encoder** out) {
	return guard([&] {
		if (!out) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		check_dims(sx, sy, sz, dtype_bytes, 0);
		select_device(device);
		std::unique_ptr<ckl_encoder> e(new ckl_encoder());
		e->device = device;
		e->dtype_bytes = dtype_bytes;
		CKL_HIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
		{
			// the label stream ahead of the trail stream: its many small kernels should be through before
			// the serial walk (k_trail_walk, one wavefront per slice) starts, whose step time suffers beside them
			int lo = 0, hi = 0;
			CKL_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
			CKL_HIP(hipStreamCreateWithPriority(&e->stream2, hipStreamNonBlocking, hi));
		}
		CKL_HIP(hipEventCreate(&e->ev0));
		CKL_HIP(hipEventCreate(&e->ev1));
		CKL_HIP(hipEventCreate(&e->evd0));
		CKL_HIP(hipEventCreate(&e->evd1));
		CKL_HIP(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
		CKL_HIP(hipEventCreateWithFlags(&e->ev_prezero, hipEventDisableTiming));
		*out = e.release();
	});
}

int ckl_encoder_run(
	ckl_encoder* e, const void* labels_device, int64_t sx, int64_t sy, int64_t sz,
	int allow_pins, int fortran_order, uint64_t markov_model_order,
	int optimize_pins, int auto_bgcolor, int64_t manual_bgcolor,
	const ckl_encode_overrides* overrides, uint8_t** out, uint64_t* out_len
) {
	return guard([&] {
		if (!e || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		check_dims(sx, sy, sz, e->dtype_bytes, 0);
		if (markov_model_order > 15) throw Error(CKL_ERR_ARG, "crackle_amd: markov_model_order must be in [0, 15]");
		enter(e);
		drain_host_copy(*e);      // the previous run's codes are still on their way out of d_codes_out
		const auto t_run0 = std::chrono::steady_clock::now();
		const EncodeRequest req = { allow_pins != 0, fortran_order != 0, markov_model_order, optimize_pins != 0, auto_bgcolor != 0, manual_bgcolor, overrides };
		with_label_type(e->dtype_bytes, [&](auto t) {
			encode_typed(*e, static_cast<const typename decltype(t)::type*>(labels_device), sx, sy, sz, req, out, out_len);
		});
		if (getenv("CKL_PROFILE")) {
			fprintf(stderr, "[ckl encoder_run ms] encode=%.2f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_run0).count());
		}
	});
}

int ckl_reencode_markov(const uint8_t* buf, uint64_t n, int markov_model_order, int device, uint8_t** out, uint64_t* out_len) {
	return guard([&] {
		if (!buf || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		select_device(device);
		reencode_markov(buf, n, markov_model_order, device, out, out_len);
	});
}

int ckl_encoder_defer_codes(ckl_encoder* e, int defer) {
	if (!e) { set_last_error("crackle_amd: null encoder"); return CKL_ERR_ARG; }
	e->defer_codes = defer != 0;
	return CKL_OK;
}

int ckl_encoder_async_host_copy(ckl_encoder* e, int on) {
	if (!e) { set_last_error("crackle_amd: null encoder"); return CKL_ERR_ARG; }
	e->async_host_copy = on != 0;
	return CKL_OK;
}

int ckl_encoder_host_wait(ckl_encoder* e) {
	return guard([&] {
		if (!e) throw Error(CKL_ERR_ARG, "crackle_amd: null encoder");
		if (e->host_copy_pending) select_device(e->device);
		drain_host_copy(*e);
	});
}

int ckl_encoder_keep_device_stream(ckl_encoder* e, int keep) {
	if (!e) { set_last_error("crackle_amd: null encoder"); return CKL_ERR_ARG; }
	e->keep_device_stream = keep != 0;
	return CKL_OK;
}

int ckl_encoder_device_stream(const ckl_encoder* e, const uint8_t** stream_device, uint64_t* n_bytes) {
	if (!e || !stream_device || !n_bytes) { set_last_error("crackle_amd: null argument"); return CKL_ERR_ARG; }
	if (!e->device_stream_bytes) { set_last_error("crackle_amd: no device-resident stream (ckl_encoder_keep_device_stream before the run)"); return CKL_ERR_ARG; }
	*stream_device = e->d_stream_out.p;
	*n_bytes = e->device_stream_bytes;
	return CKL_OK;
}

int ckl_encoder_codes_to_host(ckl_encoder* e, uint8_t* dst_host, uint64_t capacity, uint64_t* n_bytes) {
	return guard([&] {
		if (!e || !n_bytes) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		*n_bytes = e->last_codes_total;
		if (e->last_codes_total == 0) return;
		if (!dst_host || capacity < e->last_codes_total) throw Error(CKL_ERR_ARG, "crackle_amd: code buffer too small: need " + std::to_string(e->last_codes_total) + " bytes");
		select_device(e->device);
		if (e->async_host_copy) {
			// (the run that left the codes has drained e->stream: nothing to order after)
			if (!e->stream_copy) CKL_HIP(hipStreamCreateWithFlags(&e->stream_copy, hipStreamNonBlocking));
			CKL_HIP(hipMemcpyAsync(dst_host, e->d_codes_out.p, e->last_codes_total, hipMemcpyDeviceToHost, e->stream_copy));
			e->host_copy_pending = true;
			return;
		}
		CKL_HIP(hipMemcpyAsync(dst_host, e->d_codes_out.p, e->last_codes_total, hipMemcpyDeviceToHost, e->stream));
		CKL_HIP(hipStreamSynchronize(e->stream));
	});
}

int ckl_encoder_stats(
	ckl_encoder* e, const void* labels_device, int64_t sx, int64_t sy, int64_t sz,
	uint64_t* max_label, uint64_t* pixel_pairs, uint64_t* first_voxel, uint64_t* last_voxel
) {
	return guard([&] {
		enter(e);
		check_dims(sx, sy, sz, e->dtype_bytes, 0);
		const uint64_t voxels = static_cast<uint64_t>(sx) * sy * sz;
		VolumeStats st;
		e->planes_for = nullptr;
		if (voxels > 0) {
			// the label-plane pass yields max / pairs from the same read and leaves the planes for
			// the ckl_encoder_run that follows; the slab's first and last voxel come back with its counts
			// (they were two blocking copies behind it)
			uint64_t f = 0, l = 0;
			const uint8_t* base = static_cast<const uint8_t*>(labels_device);
			// the two copies land in this frame: whatever leaves it early (planes_pass throws on an allocation or a HIP
			// error) waits for them first
			struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{ e->stream };
			CKL_HIP(hipMemcpyAsync(&f, base, e->dtype_bytes, hipMemcpyDeviceToHost, e->stream));
			CKL_HIP(hipMemcpyAsync(&l, base + (voxels - 1) * e->dtype_bytes, e->dtype_bytes, hipMemcpyDeviceToHost, e->stream));
			planes_pass_any(*e, labels_device, sx, sy, sz, &st);
			CKL_HIP(hipStreamSynchronize(e->stream));      // (planes_pass has waited for the stream already: this returns at once)
			st.first = f; st.last = l;
			e->planes_for = labels_device;
			e->planes_stats = st;
			e->planes_dims[0] = sx; e->planes_dims[1] = sy; e->planes_dims[2] = sz;
		}
		if (max_label) *max_label = st.max_label;
		if (pixel_pairs) *pixel_pairs = st.pairs;
		if (first_voxel) *first_voxel = st.first;
		if (last_voxel) *last_voxel = st.last;
	});
}

int ckl_encoder_markov_stats(
	ckl_encoder* e, const void* labels_device, int64_t sx, int64_t sy, int64_t sz,
	int crack_format, uint64_t markov_model_order, uint32_t* hist
) {
	return guard([&] {
		if (!e || !hist) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		check_dims(sx, sy, sz, e->dtype_bytes, 0);
		if (markov_model_order == 0 || markov_model_order > 13) throw Error(CKL_ERR_ARG, "crackle_amd: markov_model_order must be in [1, 13]");
		enter(e);
		const size_t rows = static_cast<size_t>(1) << (2 * markov_model_order);
		std::vector<uint32_t> h(rows * 4, 0);
		if (static_cast<uint64_t>(sx) * sy * sz > 0) {
			CrackRequest crq;
			crq.goal = CrackGoal::HISTOGRAM;
			crq.permissible = crack_format == PERMISSIBLE;
			crq.markov_order = static_cast<int>(markov_model_order);
			const bool cached = planes_cached(*e, labels_device, sx, sy, sz);
			if (!cached) planes_pass_any(*e, labels_device, sx, sy, sz, nullptr);
			e->trail_for = nullptr;
			graph_pass(*e, sx, sy, sz, graph_format(crq.permissible));
			h = crack_pass(*e, sx, sy, sz, crq).hist;
			if (cached) { e->trail_for = labels_device; e->trail_perm = crq.permissible; e->trail_order = crq.markov_order; }      // (only beside cached planes: the run checks both)
		}
		memcpy(hist, h.data(), h.size() * sizeof(uint32_t));
	});
}

// shared by ckl_encoder_components / ckl_encoder_components_device: components of the slab, ids
// painted into cc_device (null: the session's own volume); returns where they are
static uint32_t* encoder_components(ckl_encoder* e, const void* labels_device, int64_t sx, int64_t sy, int64_t sz, uint32_t id_base, uint32_t* cc_device, uint32_t* ncomp_host) {
	check_dims(sx, sy, sz, e->dtype_bytes, 0);
	enter(e);
	const uint64_t voxels = static_cast<uint64_t>(sx) * sy * sz;
	if (voxels == 0) return cc_device;
	FlatResult fr;
	if (!planes_cached(*e, labels_device, sx, sy, sz)) planes_pass_any(*e, labels_device, sx, sy, sz, nullptr);
	flat_enqueue(*e, labels_device, sx, sy, sz, true, false);      // (the paint below reads the run tables)
	flat_collect(*e, labels_device, e->dtype_bytes, sx, sy, sz, fr);
	if (fr.total + id_base > 0xFFFFFFFFull) throw Error(CKL_ERR_RUNTIME, "crackle_amd: too many components");
	if (!cc_device) { e->d_cc_volume.ensure(voxels); cc_device = e->d_cc_volume.p; }
	paint_components(*e, sx, sy, sz, id_base, cc_device);
	for (int64_t z = 0; z < sz; z++) ncomp_host[z] = fr.ncomp[z];
	return cc_device;
}

int ckl_encoder_components(
	ckl_encoder* e, const void* labels_device, int64_t sx, int64_t sy, int64_t sz,
	uint32_t id_base, uint32_t* cc_host, uint32_t* ncomp_host
) {
	return guard([&] {
		if (!e || !cc_host || !ncomp_host) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		const uint32_t* cc = encoder_components(e, labels_device, sx, sy, sz, id_base, nullptr, ncomp_host);
		const uint64_t voxels = static_cast<uint64_t>(sx) * sy * sz;
		if (voxels) CKL_HIP(hipMemcpyAsync(cc_host, cc, voxels * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream2));
		CKL_HIP(hipStreamSynchronize(e->stream2));
	});
}

int ckl_encoder_components_device(
	ckl_encoder* e, const void* labels_device, int64_t sx, int64_t sy, int64_t sz,
	uint32_t id_base, uint32_t* cc_device, uint32_t* ncomp_host
) {
	return guard([&] {
		if (!e || !cc_device || !ncomp_host) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		encoder_components(e, labels_device, sx, sy, sz, id_base, cc_device, ncomp_host);
		CKL_HIP(hipStreamSynchronize(e->stream2));
	});
}

int ckl_encoder_last_timing(const ckl_encoder* e, float* pipeline_ms, float* dominant_kernel_ms) {
	if (!e) { set_last_error("crackle_amd: null encoder"); return CKL_ERR_ARG; }
	if (pipeline_ms) *pipeline_ms = e->pipeline_ms;
	if (dominant_kernel_ms) *dominant_kernel_ms = e->dominant_ms;
	return CKL_OK;
}

int ckl_encoder_walk_paths(ckl_encoder* e, uint32_t* fast_slices, uint32_t* compiled_slices) {
	return guard([&] {
		if (!e) throw Error(CKL_ERR_ARG, "crackle_amd: null encoder");
		uint32_t fast = 0, plain = 0;
		const size_t ns = e->last_trail_slices;
		if (ns && e->t_counters.p) {
			select_device(e->device);
			std::vector<uint32_t> nev(ns);
			CKL_HIP(hipMemcpy(nev.data(), e->t_counters.p + 5 * ns, ns * sizeof(uint32_t), hipMemcpyDeviceToHost));      // n_events, flagged with the event format
			for (uint32_t v : nev) { if (v & (kEvFormatAddr12 | kEvWalkWide)) fast++; else if (v) plain++; }
		}
		if (fast_slices) *fast_slices = fast;
		if (compiled_slices) *compiled_slices = plain;
	});
}

int ckl_encoder_emit_path(const ckl_encoder* e, int* fused, uint64_t* lds_bytes) {
	if (!e) { set_last_error("crackle_amd: null encoder"); return CKL_ERR_ARG; }
	if (fused) *fused = e->emit_fused ? 1 : 0;
	if (lds_bytes) *lds_bytes = e->emit_lds;
	return CKL_OK;
}

int ckl_encoder_walk_step_kinds(ckl_encoder* e, uint32_t* counts, uint32_t max_slices, uint32_t* n_slices) {
	return guard([&] {
		if (!e || !counts || !n_slices) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		const size_t ns = e->last_trail_slices;
		*n_slices = static_cast<uint32_t>(ns);
		if (!ns || !e->t_counters.p || !e->t_events.p) { *n_slices = 0; return; }
		if (ns > max_slices) throw Error(CKL_ERR_ARG, "crackle_amd: counts holds fewer slices than the last run had");
		select_device(e->device);
		DevBuf<uint32_t> d_counts;
		d_counts.ensure(ns * 5);
		hipLaunchKernelGGL(k_trail_step_kinds, dim3(static_cast<uint32_t>(ns)), dim3(kBlock), 0, e->stream, e->t_events.p, e->t_ibase.p, e->t_counters.p + 5 * ns, d_counts.p);
		CKL_HIP(hipMemcpyAsync(counts, d_counts.p, ns * 5 * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
		CKL_HIP(hipStreamSynchronize(e->stream));
	});
}

void ckl_encoder_destroy(ckl_encoder* e) { delete e; }

int ckl_compress(
	const void* labels, int labels_mem, int dtype_bytes, int is_signed,
	int64_t sx, int64_t sy, int64_t sz,
	int allow_pins, int fortran_order, uint64_t markov_model_order,
	int optimize_pins, int auto_bgcolor, int64_t manual_bgcolor,
	int device, uint8_t** out, uint64_t* out_len
) {
	ckl_encoder* e = nullptr;
	try {
		check_dims(sx, sy, sz, dtype_bytes, is_signed);
		if (!out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		if (static_cast<uint64_t>(sx) * sy * sz == 0) {
			// crackle.hpp:96-98: an empty volume is just the 29-byte header; nothing to compute (its statistics are all 0)
			hand_out(header_bytes(stream_header(dtype_bytes, sx, sy, sz, VolumeStats(), allow_pins != 0, fortran_order != 0, markov_model_order, nullptr)), OutAlloc::MALLOC, out, out_len);
			return CKL_OK;
		}
	}
	catch (const Error& err) { set_last_error(err.what()); return err.status; }
	const int rc = ckl_encoder_create(sx, sy, sz, dtype_bytes, device, &e);
	if (rc != CKL_OK) return rc;
	DevBuf<uint8_t> tmp;      // (in front of the session: ~ckl_encoder waits for its streams before the labels go back to the pool, also when the run failed)
	const EncoderPtr owner(e);
	return guard([&]() -> int {
		const uint64_t bytes = static_cast<uint64_t>(sx) * sy * sz * dtype_bytes;
		const void* dev_labels = labels;
		if (labels_mem == CKL_MEM_HOST && bytes) {
			if (!labels) throw Error(CKL_ERR_ARG, "crackle_amd: null labels");
			tmp.ensure(bytes);
			CKL_HIP(hipMemcpy(tmp.p, labels, bytes, hipMemcpyHostToDevice));
			dev_labels = tmp.p;
		}
		return ckl_encoder_run(e, dev_labels, sx, sy, sz, allow_pins, fortran_order, markov_model_order,
			optimize_pins, auto_bgcolor, manual_bgcolor, nullptr, out, out_len);
	});
}

}  // extern "C"
