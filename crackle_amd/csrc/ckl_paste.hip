// ckl_paste: an x, y, z box written into a stream (the reference's CrackleArray.__setitem__,
// crackle/array.py:287-340, decodes the slices of the z-range to the host, lets numpy assign, compresses
// the slab and splices it in with zsplit / zstack).  Here the slab never leaves HBM: a decode session
// paints slices [z0, z1) x fastest into a library-owned buffer, k_paste_box writes the box (or a fill
// value) into it, an encode session reads it in place, and only the stream's bytes and the box cross
// the link.  Two cases fix the bytes:
//   splice     version 1, FLAT labels, [z0, z1) not the whole depth: the slab's stream is forced to the
//              input's crack format, FLAT labels, markov order and markov MODEL, so ckl_zstack takes the
//              untouched slices' z-index entries, crack codes and crcs from ckl_zsplit's ranges as they are.
//              (The reference compresses the slab with defaults — another crack format makes its zstack
//              raise, operations.py:480 — and brings every part to order 0 first, operations.py:455-457.)
//   re-encode  everything else (whole depth, pin labels, version 0: ckl_zsplit serves FLAT version 1
//              only): the whole volume is the slab and its stream is ckl_compress's, every decision free.
#include "ckl_decoder.hpp"

#include <algorithm>

namespace ckl {

using namespace dev;

struct PasteArgs {
	uint32_t sx, sy;              // the slab's slices
	uint32_t x0, x1, y0, y1;      // the box in pixels of a slice, x0 < x1 <= sx, y0 < y1 <= sy
	uint32_t z0, wz;              // its first slice IN THE SLAB and its depth, z0 + wz <= slices of the slab
	uint32_t fortran_order;       // the box is x fastest (else z fastest)
	uint32_t has_box;             // 0: every voxel of the box becomes `value`
	uint64_t value;
};

// The slab is x fastest and a box row starts at element x0 + sx * (y + sy * z): aligned to nothing but the
// element.  Small scattered stores run at the L2s' request rate, not their byte rate (k_paint_window,
// tools/micro/store_bw.hip), so a thread takes chunks that are 16 bytes IN THE SLAB: whole chunks are one
// vector store, the head and the tail of a row go element by element, and consecutive threads take
// consecutive chunks of a row.  The source row is read at whatever alignment it has; a box that is not
// fortran_order is z fastest and read with a stride: correct, not fast.
// grid-stride over (wx / V + 1 chunks) * wy * wz, block = kBlock
template <typename LABEL>
__global__ void __launch_bounds__(kBlock) k_paste_box(LABEL* __restrict__ slab, const LABEL* __restrict__ box, PasteArgs a) {
	constexpr uint32_t V = 16 / sizeof(LABEL);      // voxels of a chunk
	struct alignas(16) Chunk { LABEL v[V]; };
	const uint32_t wx = a.x1 - a.x0, wy = a.y1 - a.y0;
	const uint32_t cpr = (wx + V - 1u) / V + 1u;      // a row has a partial chunk in front when it does not start on 16 bytes
	const uint64_t nchunks = static_cast<uint64_t>(wy) * a.wz * cpr;
	const uint64_t base = reinterpret_cast<uintptr_t>(slab) / sizeof(LABEL);
	const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
	for (uint64_t ci = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; ci < nchunks; ci += stride) {
		const uint64_t row = ci / cpr;
		const uint32_t c = static_cast<uint32_t>(ci - row * cpr);
		const uint32_t zr = static_cast<uint32_t>(row / wy), yr = static_cast<uint32_t>(row - static_cast<uint64_t>(zr) * wy);
		const uint64_t d0 = a.x0 + static_cast<uint64_t>(a.sx) * ((a.y0 + yr) + static_cast<uint64_t>(a.sy) * (a.z0 + zr));      // the row's first element in the slab
		const uint32_t mis = static_cast<uint32_t>((base + d0) % V);
		const uint32_t lo = c ? c * V - mis : 0u;
		const uint32_t hi = min(wx, (c + 1u) * V - mis);
		if (lo >= hi) continue;
		const uint64_t src0 = (static_cast<uint64_t>(zr) * wy + yr) * wx;      // fortran_order: the row's first element in the box
		auto voxel = [&](uint32_t e) -> LABEL {      // voxel e of the row
			if (!a.has_box) return static_cast<LABEL>(a.value);
			return a.fortran_order ? box[src0 + e] : box[(static_cast<uint64_t>(e) * wy + yr) * a.wz + zr];
		};
		LABEL* dst = slab + d0 + lo;
		if (hi - lo == V) {
			Chunk ch;
			if (a.has_box && a.fortran_order) __builtin_memcpy(&ch, box + src0 + lo, sizeof(Chunk));
			else {
#pragma unroll
				for (uint32_t j = 0; j < V; j++) ch.v[j] = voxel(lo + j);
			}
			*reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&ch);
		}
		else {
			// head or tail of the row (a loop of its own on purpose: unrolled beside the vector store, the compiler
			// merges the two and splits the 16-byte store to share its last element's store with this one)
#pragma nounroll
			for (uint32_t e = lo; e < hi; e++) dst[e - lo] = voxel(e);
		}
	}
}

}  // namespace ckl

using namespace ckl;

namespace {

// a block another entry point handed out (ckl_free releases every kind)
struct Owned {
	uint8_t* p = nullptr;
	uint64_t n = 0;
	Owned() = default;
	Owned(const Owned&) = delete;
	Owned& operator=(const Owned&) = delete;
	~Owned() { if (p) ckl_free(p); }
};

void launch_paste(void* slab, const void* box, const PasteArgs& a, int width, hipStream_t s) {
	const uint64_t v = 16u / static_cast<uint32_t>(width);
	const uint64_t nchunks = static_cast<uint64_t>(a.y1 - a.y0) * a.wz * ((a.x1 - a.x0 + v - 1) / v + 1);
	const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>((nchunks + kBlock - 1) / kBlock, 1u << 20)));
	with_label_type(width, [&](auto t) {
		typedef typename decltype(t)::type LABEL;
		hipLaunchKernelGGL(k_paste_box<LABEL>, grid, dim3(kBlock), 0, s, static_cast<LABEL*>(slab), static_cast<const LABEL*>(box), a);
	});
}

// The one label of a stream that holds a single one (FLAT: a unique list of one entry; pins: an empty list, all
// background colour).  The Python layer answers such streams on the host (codec.decompress_range) and never
// shows them to a decode session: here the slab is filled by the paste kernel instead.
bool single_label(const Header& h, const uint8_t* buf, uint64_t n, uint64_t* label) {
	if (!h.layout_fits(n)) throw Error(CKL_ERR_RUNTIME, "crackle: Unable to read past end of buffer.");
	const uint8_t* lb = buf + h.header_bytes() + h.grid_index_bytes();
	const uint64_t sw = static_cast<uint64_t>(h.stored_data_width);
	if (h.label_format == FLAT) {
		if (h.num_label_bytes < 8 + sw || rd_le(lb, 8) != 1) return false;
		*label = rd_le(lb + 8, static_cast<int>(sw));
		return true;
	}
	if (h.num_label_bytes < sw + 8 || rd_le(lb + sw, 8) != 0) return false;
	*label = rd_le(lb, static_cast<int>(sw));
	return true;
}

}  // namespace

extern "C" int ckl_paste(
	const uint8_t* buf, uint64_t n, const void* box, int box_mem, int has_box, uint64_t value,
	int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1,
	int device, uint8_t** out, uint64_t* out_len
) {
	return guard([&]() -> int {
		if (!buf || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		*out = nullptr; *out_len = 0;
		if (n < Header::kBytesV0) throw Error(CKL_ERR_FORMAT, "crackle: Input too small to be a valid stream. Bytes: " + std::to_string(n));
		const Header h = Header::parse(buf, n);
		if (h.is_signed) throw Error(CKL_ERR_ARG, "Signed integer data types are not currently supported.");
		check_box_axis("paste", "x", x0, x1, h.sx);
		check_box_axis("paste", "y", y0, y1, h.sy);
		check_box_axis("paste", "z", z0, z1, h.sz);
		const int w = h.data_width;
		if (!has_box && w < 8 && (value >> (8 * w))) throw Error(CKL_ERR_ARG, "crackle_amd: paste: value " + std::to_string(value) + " does not fit the stream's " + std::to_string(w) + "-byte labels");
		if (box_mem != CKL_MEM_HOST && box_mem != CKL_MEM_DEVICE) throw Error(CKL_ERR_ARG, "crackle_amd: paste: box_mem must be CKL_MEM_HOST or CKL_MEM_DEVICE");
		const uint64_t box_bytes = static_cast<uint64_t>(x1 - x0) * static_cast<uint64_t>(y1 - y0) * static_cast<uint64_t>(z1 - z0) * static_cast<uint64_t>(w);
		if (box_bytes == 0) {
			// an empty box: the stream as it is, no device
			uint8_t* o = static_cast<uint8_t*>(malloc(n));
			if (!o) throw Error(CKL_ERR_RUNTIME, "crackle_amd: out of host memory");
			memcpy(o, buf, n);
			*out = o; *out_len = n;
			return CKL_OK;
		}
		if (has_box && !box) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");

		const bool splice = h.format_version == 1 && h.label_format == FLAT && !(z0 == 0 && z1 == static_cast<int64_t>(h.sz));
		const int64_t s0 = splice ? z0 : 0, s1 = splice ? z1 : static_cast<int64_t>(h.sz);
		const uint64_t sxy = static_cast<uint64_t>(h.sx) * h.sy;
		const uint32_t ns = static_cast<uint32_t>(s1 - s0);
		const uint64_t slab_bytes = sxy * ns * static_cast<uint64_t>(w);
		uint64_t only = 0;
		const bool single = single_label(h, buf, n, &only);
		// the model as the encoder's override takes it, symbol -> rank (the stream stores rank -> symbol)
		std::vector<uint8_t> model;
		if (splice && h.markov_model_order > 0) {
			const uint8_t* stored = buf + h.header_bytes() + h.grid_index_bytes() + h.num_label_bytes;
			const std::vector<uint8_t> by_rank = markov_model_from_stored(stored, h.markov_model_bytes(), h.markov_model_order);
			model.resize(by_rank.size());
			for (size_t r = 0; r < by_rank.size() / 4; r++) for (uint8_t k = 0; k < 4; k++) model[r * 4 + by_rank[r * 4 + k]] = k;
		}

		select_device(device);
		DevBuf<uint8_t> slab, box_dev;
		slab.ensure(slab_bytes);
		const void* box_d = box;
		if (has_box && box_mem == CKL_MEM_HOST) {
			box_dev.ensure(box_bytes);
			CKL_HIP(hipMemcpy(box_dev.p, box, box_bytes, hipMemcpyHostToDevice));
			box_d = box_dev.p;
		}
		PasteArgs pa;
		pa.sx = h.sx; pa.sy = h.sy;
		pa.fortran_order = h.fortran_order ? 1u : 0u;
		{
			// 1. the slab: slices [s0, s1), x fastest whatever the stream's fortran_order (the encoder's input layout)
			DecoderPtr dec;
			hipStream_t s = nullptr;      // (a single-label stream opens no session: the default stream, which also orders a device box behind its writer)
			if (single) {
				pa.x0 = 0; pa.x1 = h.sx; pa.y0 = 0; pa.y1 = h.sy; pa.z0 = 0; pa.wz = ns;
				pa.has_box = 0; pa.value = only;
				launch_paste(slab.p, nullptr, pa, w, s);
			}
			else {
				const int rc = open_decoder(buf, n, s0, s1, device, dec);
				if (rc != CKL_OK) return rc;
				enter(dec.get());
				RunRequest rq = { Goal::PAINT, slab.p, slab_bytes };
				rq.x_fastest = true;
				decoder_run(*dec, rq);      // a damaged slice of [s0, s1) raises here, as for a decode
				s = dec->stream;
			}
			// 2. the box, behind the paint on the same stream
			pa.x0 = static_cast<uint32_t>(x0); pa.x1 = static_cast<uint32_t>(x1); pa.y0 = static_cast<uint32_t>(y0); pa.y1 = static_cast<uint32_t>(y1);
			pa.z0 = static_cast<uint32_t>(z0 - s0); pa.wz = static_cast<uint32_t>(z1 - z0);
			pa.has_box = has_box ? 1u : 0u; pa.value = value;
			launch_paste(slab.p, box_d, pa, w, s);
			// the encoder runs on streams of its own: it starts when the slab is complete
			CKL_HIP(hipStreamSynchronize(s));
			CKL_HIP(hipGetLastError());
		}      // (the decode session's scratch goes back to the pool before the encoder asks for its own)
		box_dev.release();

		// 3. the slab's stream
		ckl_encoder* raw = nullptr;
		int rc = ckl_encoder_create(h.sx, h.sy, ns, w, device, &raw);
		if (rc != CKL_OK) return rc;
		EncoderPtr enc(raw);
		ckl_encode_overrides ov = {};
		ov.force_crack_format = h.crack_format;
		ov.force_label_format = FLAT;
		ov.has_model = model.empty() ? 0 : 1;
		ov.model = model.empty() ? nullptr : model.data();
		Owned mid;
		rc = ckl_encoder_run(enc.get(), slab.p, h.sx, h.sy, ns, 0, h.fortran_order ? 1 : 0, static_cast<uint64_t>(h.markov_model_order), 0, 1, 0,
			splice ? &ov : nullptr, &mid.p, &mid.n);
		if (rc != CKL_OK) return rc;
		enc.reset();
		slab.release();
		if (!splice) {
			*out = mid.p; *out_len = mid.n;
			mid.p = nullptr;
			return CKL_OK;
		}

		// 4. the untouched slices around it, as ckl_zsplit copies them
		Owned before, after;
		if (z0 > 0) {
			rc = ckl_zsplit(buf, n, 0, z0, &before.p, &before.n);
			if (rc != CKL_OK) return rc;
		}
		if (z1 < static_cast<int64_t>(h.sz)) {
			rc = ckl_zsplit(buf, n, z1, h.sz, &after.p, &after.n);
			if (rc != CKL_OK) return rc;
		}
		std::vector<const uint8_t*> bufs;
		std::vector<uint64_t> lens;
		for (const Owned* o : { &before, &mid, &after }) if (o->p) { bufs.push_back(o->p); lens.push_back(o->n); }
		return ckl_zstack(bufs.data(), lens.data(), bufs.size(), out, out_len);
	});
}
