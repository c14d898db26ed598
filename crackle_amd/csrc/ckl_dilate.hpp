// ckl_dilate: the labels of a stream grown by one voxel, without its voxels.  A voxel whose label is not 0 keeps it.  A
// voxel with label 0 looks at the neighbours of ckl_erode's structuring element (6, 18 or 26 offsets) that lie inside
// the volume and carry a label other than 0: without any it stays 0, otherwise it takes the label that occurs most often
// among them, and among labels tied for most often the SMALLEST, compared as unsigned 64-bit values (this project's
// rule).  Neighbours outside the volume do not exist.  One iteration.
//
// A gained voxel's label is not a function of its run, so beside the run tables the label stage gets a second source:
//   gain        [nslices][plane_words]  bit x set: the pixel is 0 and some counted neighbour is not (it is "gained")
//   gain_off    [nslices][plane_words]  where the word's gained pixels stand in gain_label (64-bit)
//   gain_label  [gained]                the label of every gained pixel; pixel x of a word is at gain_off + popc(gain & bits below x)
// The kernels, in launch order:
//   k_erode_run_labels   (ckl_erode.hpp) one label per run
//   k_dilate_nonzero     per 32-pixel word the bit plane N: label != 0, one label fetch per run
//   k_dilate_gain        gain from N of the word's (up to) nine rows and their neighbouring words; gain_off: an exclusive
//                        scan inside the workgroup on top of a base the workgroup takes from one 64-bit cursor.  The order
//                        in which workgroups take their bases differs from call to call; nothing but the position inside
//                        gain_label depends on it, and gain_label is only ever read through gain_off.
//   -- the cursor's final value, the number of gained pixels, crosses to the host, which sizes gain_label (0: the
//      call goes on as a recompress, nothing below is launched) --
//   k_dilate_mode        per gained pixel the neighbours' labels through the run tables, their mode -> gain_label (a
//                        thread per gained pixel of the workgroup's 256 words)
//   k_dilate_planes      the encoder's V and H planes of the dilated labels, their per-slice counts, the wrap-around pairs
// With N(dy, dz) the plane N of row (y + dy, z + dz), F the OR of the four face rows (|dy| + |dz| = 1), D the OR of the
// four diagonal rows, side(X) = X(x - 1) | X(x + 1) and ext(X) = X | side(X), both inside the row (a row's first and last
// pixel have no neighbour in the adjacent row's last or first pixel):
//    6:  gain = ~N & (side(N) | F)
//   18:  gain = ~N & (side(N) | ext(F) | D)
//   26:  gain = ~N & (side(N) | ext(F | D))
#pragma once

#include "ckl_erode.hpp"

namespace ckl {
namespace dev {

struct DilateArgs {
	uint32_t connectivity;      // 6, 18, 26
	uint32_t nslices;
};

// One thread per word: N.  Bits at or past sx are 0.  grid = (ceil(plane_words / 256), nslices)
__global__ void __launch_bounds__(kBlock) k_dilate_nonzero(RunLabels t, const uint64_t* __restrict__ run_label, uint32_t* __restrict__ planeN) {
	const RunGeom& g = t.g;
	const uint32_t zi = blockIdx.y;
	const uint64_t i = this_word();
	if (i >= g.plane_words) return;
	const PlaneWord pw(g, zi, i);
	uint32_t same_as_before;      // (unused)
	planeN[pw.at] = nonzero_bits(t, run_label, zi, pw, g.breaks(zi, pw.y, pw.w), same_as_before);
}

// One thread per word: gain and gain_off (header comment).  *cursor zeroed by the host; afterwards it holds the number of
// gained pixels.  No thread leaves early: the scan is the workgroup's.  grid = (ceil(plane_words / 256), nslices)
__global__ void __launch_bounds__(kBlock) k_dilate_gain(
	RunGeom g, DilateArgs a, const uint32_t* __restrict__ planeN, uint32_t* __restrict__ gain, uint64_t* __restrict__ gain_off, unsigned long long* __restrict__ cursor
) {
	__shared__ uint32_t s_scan[kWaves];
	__shared__ unsigned long long s_base;
	const uint32_t zi = blockIdx.y;
	const uint64_t i = this_word();
	const bool live = i < g.plane_words;
	const uint64_t at = zi * g.plane_words + i;
	uint32_t gw = 0;
	if (live) {
		const PlaneWord pw(g, zi, i);
		const uint32_t y = pw.y, w = pw.w;
		const bool first = w == 0u, last = w + 1u == g.row_words;
		// the word of row (y + dy, zi + dz), the last bit of the word before it and the first bit of the word after it
		auto row = [&](int dy, int dz, uint32_t& c, uint32_t& l, uint32_t& r) {
			const int64_t yn = static_cast<int64_t>(y) + dy, zn = static_cast<int64_t>(zi) + dz;
			if (yn < 0 || yn >= static_cast<int64_t>(g.sy) || zn < 0 || zn >= static_cast<int64_t>(a.nslices)) return;
			const uint64_t an = static_cast<uint64_t>(zn) * g.plane_words + static_cast<uint64_t>(yn) * g.row_words + w;
			c |= planeN[an];
			if (!first) l |= planeN[an - 1] >> 31;
			if (!last) r |= planeN[an + 1] << 31;
		};
		uint32_t nc = 0, nl = 0, nr = 0, fc = 0, fl = 0, fr = 0, dc = 0, dl = 0, dr = 0;
		row(0, 0, nc, nl, nr);
		row(-1, 0, fc, fl, fr); row(1, 0, fc, fl, fr); row(0, -1, fc, fl, fr); row(0, 1, fc, fl, fr);
		if (a.connectivity != 6u) { row(-1, -1, dc, dl, dr); row(1, -1, dc, dl, dr); row(-1, 1, dc, dl, dr); row(1, 1, dc, dl, dr); }
		auto side = [](uint32_t c, uint32_t l, uint32_t r) { return (c << 1) | l | (c >> 1) | r; };
		uint32_t near = side(nc, nl, nr);
		if (a.connectivity == 6u) near |= fc;
		else if (a.connectivity == 18u) near |= fc | side(fc, fl, fr) | dc;
		else near |= fc | dc | side(fc | dc, fl | dl, fr | dr);
		gw = near & ~nc & pw.valid;
		gain[at] = gw;
	}
	uint32_t v[1] = { static_cast<uint32_t>(__popc(gw)) }, total[1];
	block_excl_add<1>(v, total, s_scan);
	if (threadIdx.x == 0) s_base = total[0] ? atomicAdd(cursor, static_cast<unsigned long long>(total[0])) : 0ull;
	__syncthreads();
	if (live) gain_off[at] = s_base + v[0];
}

// One workgroup per 256 words, one thread per gained pixel of those words: the labels of the counted neighbours, their
// mode, the store into gain_label.  The words' gained pixels are numbered by a scan of the popcounts inside the
// workgroup, and thread k takes the pixels k, k + 256, ...: it finds the pixel's word by a binary search of the scan
// and the pixel as the word's j-th set bit.  (A thread per word, looping over its bits, was built first: cell faces
// that lie across y or z fill whole words with gained pixels while most words hold one or two or none, and a wave
// waited for its fullest word.  It took 8.1 and 16.6 ms at C2 against the figures in DESIGN.md.)
// In a neighbour row the columns x - 1, x, x + 1 lie in consecutive runs, run(x) - break(x), run(x),
// run(x) + break(x + 1), so a row costs one label fetch per run it shows, not one per pixel, and a row in which N shows
// nothing to count costs two words.  A pixel first fetches the labels of all its rows (the row loop is unrolled: the
// loads are independent and in flight together), then counts them: the thread keeps the distinct labels it has seen and
// their counts in a column of LDS of its own (up to 26 entries; usually one to three), and equal labels of a row are
// counted in one step.  Held in registers with 26 x 26 unrolled comparisons the list took 256 VGPRs and spilled.  No
// thread reads another's column.  grid = (ceil(plane_words / 256), nslices)
constexpr int kDilateNeighbours = 26;
constexpr int kDilateRows = 9;
__global__ void __launch_bounds__(kBlock) k_dilate_mode(
	RunLabels t, const uint64_t* __restrict__ run_label, DilateArgs a, const uint32_t* __restrict__ planeN, const uint32_t* __restrict__ gain,
	const uint64_t* __restrict__ gain_off, uint64_t* __restrict__ gain_label
) {
	__shared__ uint64_t s_label[kDilateNeighbours * kBlock];
	__shared__ uint8_t s_count[kDilateNeighbours * kBlock];
	__shared__ uint32_t s_gain[kBlock], s_start[kBlock], s_scan[kWaves];
	const RunGeom& g = t.g;
	const uint32_t zi = blockIdx.y;
	const uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * kBlock;
	{
		const uint64_t i = i0 + threadIdx.x;
		const uint32_t gw = i < g.plane_words ? gain[zi * g.plane_words + i] : 0u;
		uint32_t v[1] = { static_cast<uint32_t>(__popc(gw)) }, total[1];
		block_excl_add<1>(v, total, s_scan);
		s_gain[threadIdx.x] = gw;
		s_start[threadIdx.x] = v[0];
		if (threadIdx.x == 0) s_scan[0] = total[0];
	}
	__syncthreads();
	const uint32_t n_items = s_scan[0];      // at most 256 * 32
	const uint32_t reach = a.connectivity == 6u ? 1u : (a.connectivity == 18u ? 2u : 3u);
	uint64_t* const my_label = s_label + threadIdx.x;
	uint8_t* const my_count = s_count + threadIdx.x;
	for (uint32_t item = threadIdx.x; item < n_items; item += kBlock) {
		// the last word whose start is <= item (words without gained pixels share their start with the next word that has some)
		uint32_t tw = 0;
#pragma unroll
		for (uint32_t step = kBlock / 2; step >= 1u; step >>= 1) if (s_start[tw + step] <= item) tw += step;
		const uint32_t gw = s_gain[tw];
		uint32_t bits = gw;
		for (uint32_t j = item - s_start[tw]; j; j--) bits &= bits - 1u;
		const uint32_t xb = __builtin_ctz(bits);      // (bits != 0: the word has more than item - start gained pixels)
		const PlaneWord pw(g, zi, i0 + tw);
		const uint32_t y = pw.y, w = pw.w;
		const bool first = w == 0u, last = w + 1u == g.row_words;
		// the labels, row r = 3 * (dz + 1) + (dy + 1): 0 where there is nothing to count
		uint64_t ll[kDilateRows], lc[kDilateRows], lr[kDilateRows];
#pragma unroll
		for (int dz = -1; dz <= 1; dz++) {
#pragma unroll
			for (int dy = -1; dy <= 1; dy++) {
				const int r = 3 * (dz + 1) + (dy + 1);
				const uint32_t dist = static_cast<uint32_t>((dz != 0) + (dy != 0));
				const int64_t yn = static_cast<int64_t>(y) + dy, zn = static_cast<int64_t>(zi) + dz;
				ll[r] = 0; lc[r] = 0; lr[r] = 0;
				if (dist > reach || yn < 0 || yn >= static_cast<int64_t>(g.sy) || zn < 0 || zn >= static_cast<int64_t>(a.nslices)) continue;
				const uint32_t zr = static_cast<uint32_t>(zn), yr = static_cast<uint32_t>(yn);
				const uint64_t an = zr * g.plane_words + static_cast<uint64_t>(yr) * g.row_words + w;
				const uint32_t n = planeN[an];
				const bool c = dist != 0u && ((n >> xb) & 1u);      // (dist = 0 is the pixel's own row: the pixel itself is 0)
				bool l = false, rr = false;
				if (dist + 1u <= reach) {                           // x - 1 and x + 1 count one step further out than x
					l = xb ? (n >> (xb - 1u)) & 1u : (first ? 0u : planeN[an - 1] >> 31);
					rr = xb < 31u ? (n >> (xb + 1u)) & 1u : (last ? 0u : planeN[an + 1] & 1u);
				}
				if (c | l | rr) {
					const SliceRunLabels lab(t, run_label, zr);
					const uint32_t b = g.breaks(zr, yr, w);
					const uint32_t rx = t.word_base[an] + __popc(b & mask_le(xb)) - 1u;
					const uint32_t b0 = (b >> xb) & 1u;
					const uint32_t b1 = xb < 31u ? (b >> (xb + 1u)) & 1u : (last ? 0u : g.breaks(zr, yr, w + 1u) & 1u);
					const uint64_t mid = lab(rx);
					if (c) lc[r] = mid;
					if (l) ll[r] = b0 ? lab(rx - 1u) : mid;
					if (rr) lr[r] = b1 ? lab(rx + 1u) : mid;
				}
			}
		}
		// the distinct labels and their counts
		uint32_t n_list = 0;      // (at most 26: every counted neighbour adds one entry at the most)
		auto count = [&](uint64_t l, uint32_t times) {
			if (!l) return;
			uint32_t k = 0;
			while (k < n_list && my_label[k * kBlock] != l) k++;
			if (k == n_list) { my_label[k * kBlock] = l; my_count[k * kBlock] = static_cast<uint8_t>(times); n_list++; }
			else my_count[k * kBlock] = static_cast<uint8_t>(my_count[k * kBlock] + times);
		};
#pragma unroll
		for (int r = 0; r < kDilateRows; r++) {
			if (!(lc[r] | ll[r] | lr[r])) continue;
			count(lc[r], 1u + (ll[r] == lc[r]) + (lr[r] == lc[r]));
			if (ll[r] != lc[r]) count(ll[r], 1u + (lr[r] == ll[r]));
			if (lr[r] != lc[r] && lr[r] != ll[r]) count(lr[r], 1u);
		}
		// the most frequent label, the smallest of those tied (a gained pixel has a counted neighbour, so the list is not empty)
		uint64_t best = 0;
		uint32_t best_n = 0;
		for (uint32_t k = 0; k < n_list; k++) {
			const uint64_t l = my_label[k * kBlock];
			const uint32_t n = my_count[k * kBlock];
			if (n > best_n || (n == best_n && l < best)) { best = l; best_n = n; }
		}
		gain_label[gain_off[pw.at] + __popc(gw & ((1u << xb) - 1u))] = best;
	}
}

// the label of pixel (x, y) of slice zi in the dilated volume
__device__ __forceinline__ uint64_t dilated_label(const RunLabels& t, const uint64_t* run_label, uint32_t zi, uint32_t x, uint32_t y) {
	uint64_t l;
	if (t.gained(zi, x, y, l)) return l;
	return SliceRunLabels(t, run_label, zi)(t.run_at(zi, x, y));
}

// One thread per word: the dilated volume's planes V and H with the bits and the counts that k_label_planes_from_runs
// leaves (bits at or past sx, x = 0 of V and y = 0 of H stay 0; counts zeroed by the host: [nslices] bits of V,
// [nslices] bits of H, [nslices] wrap pairs).  A row of the dilated volume changes its label at a break, at a gained
// pixel and behind one; the word is cut there in the row itself and in the row above, and inside a piece both rows have
// one label each.  t carries gain, gain_off and gain_label.  grid = (ceil(plane_words / 256), nslices)
__global__ void __launch_bounds__(kBlock) k_dilate_planes(
	RunLabels t, const uint64_t* __restrict__ run_label, uint32_t* __restrict__ planeV, uint32_t* __restrict__ planeH, uint32_t* __restrict__ counts, uint32_t nslices
) {
	__shared__ uint32_t s_red[kWaves];
	const RunGeom& g = t.g;
	const uint32_t zi = blockIdx.y;
	const uint64_t i = this_word();
	uint32_t nv = 0, nh = 0, nw = 0;
	if (i < g.plane_words) {
		const auto [y, w, valid, at] = PlaneWord(g, zi, i);
		const uint64_t up = at - g.row_words;      // (used with y >= 1 only)
		const SliceRunLabels lab(t, run_label, zi);
		const uint32_t b = g.breaks(zi, y, w), bu = y ? g.breaks(zi, y - 1u, w) : 0u;
		const uint32_t gw = t.gain[at], gu = y ? t.gain[up] : 0u;
		const uint64_t off = t.gain_off[at], offu = y ? t.gain_off[up] : 0ull;
		const uint32_t rc = t.word_base[at] - 1u, ru = y ? t.word_base[up] - 1u : 0u;
		// where the label of the row may change; pixel 0 of the word is always looked up
		const uint32_t cut = b | gw | (gw << 1) | 1u;
		const uint32_t cutu = bu | gu | (gu << 1) | 1u;
		uint64_t lc = w ? dilated_label(t, run_label, zi, w * 32u - 1u, y) : 0ull, lu = 0;
		if (w == 0 && (y | zi)) {
			// the row's first pixel against the pixel before it in x-fastest order
			const uint32_t zp = y ? zi : zi - 1u, yp = y ? y - 1u : g.sy - 1u;
			nw = dilated_label(t, run_label, zp, g.sx - 1u, yp) == dilated_label(t, run_label, zi, 0u, y);
		}
		uint32_t v = 0, h = 0;
		uint32_t rest = (y ? (cut | cutu) : cut) & valid;
		while (rest) {
			const uint32_t x = __builtin_ctz(rest);
			rest &= rest - 1u;
			const uint32_t below = (1u << x) - 1u;
			if ((cut >> x) & 1u) {
				const uint64_t l = ((gw >> x) & 1u) ? t.gain_label[off + __popc(gw & below)] : lab(rc + __popc(b & mask_le(x)));
				if ((w | x) && l != lc) v |= 1u << x;
				lc = l;
			}
			if (y) {
				if ((cutu >> x) & 1u) lu = ((gu >> x) & 1u) ? t.gain_label[offu + __popc(gu & below)] : lab(ru + __popc(bu & mask_le(x)));
				if (lc != lu) h |= bits_from_to(x, rest ? __builtin_ctz(rest) : 32u);
			}
		}
		h &= valid;
		planeV[at] = v; planeH[at] = h;
		nv = __popc(v); nh = __popc(h);
	}
	add_plane_counts(nv, nh, nw, s_red, counts, nslices, zi);
}

}  // namespace dev
}  // namespace ckl
