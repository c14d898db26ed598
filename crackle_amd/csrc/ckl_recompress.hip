// crackle.operations.recompress (crackle/operations.py:664-857 decodes slabs to voxels and compresses them again), and
// erode, dilate, downsample, combine and crop, which are the same road with another volume at its end (combine: of two
// streams, through a sibling of recompress() below; crop: many volumes, the boxes of one call, from one TABLES run,
// through crop_boxes() below).  Here no voxel exists anywhere:
// a TABLES run of the decoder leaves the runs of every slice and the label of every component, a plane stage writes the
// encoder's planes and their counts from them (plain: ckl_recompress.hpp, eroded: ckl_erode.hpp, dilated:
// ckl_dilate.hpp, pooled: ckl_downsample.hpp, the one whose volume has another shape than the decoder's, combined:
// ckl_combine.hpp, the one with two decoders, cropped: ckl_crop.hpp, the one with many encoders), and
// encode_from_planes (ckl_encoder.hpp) goes on as the encoder does from cached planes, with its label stage reading the
// same tables.  The bytes are those of compress(edit(decompress(stream)), markov_model_order).
#include "ckl_encoder.hpp"
#include "ckl_decoder.hpp"
#include "ckl_recompress.hpp"
#include "ckl_erode.hpp"
#include "ckl_dilate.hpp"
#include "ckl_downsample.hpp"
#include "ckl_combine.hpp"
#include "ckl_crop.hpp"

#include <algorithm>
#include <chrono>
#include <map>
#include <tuple>

using namespace ckl;
using namespace ckl::dev;

namespace {

// what a call does to the labels on their way through
struct LabelEdit {
	enum Kind { NONE, ERODE, DILATE, POOL, COMBINE, CROP } kind = NONE;
	int connectivity = 0;          // ERODE, DILATE: 6, 18, 26
	bool keep_border = false;      // ERODE: neighbours outside the volume are ignored
	int fx = 1, fy = 1, fz = 1;    // POOL: (2, 2, 1) or (2, 2, 2)
	int rule = 0;                  // COMBINE: CKL_COMBINE_*
};

// per kind: the operation's name, and the two fields of its CKL_PROFILE line that carry the kind in their names
struct EditNames { const char *op, *planes_field, *device_field; };
constexpr EditNames kEditNames[] = {
	{ "recompress", "label_planes", "k_label_planes_from_runs_device" },
	{ "erode", "keep_planes", "k_erode_device" },
	{ "dilate", "gain_planes", "k_dilate_device" },
	{ "downsample", "pool_planes", "k_pool_device" },
	{ "combine", "merge_planes", "k_combine_device" },
	{ "crop", "crop_planes", "k_crop_device" },
};

// Device scratch of one call's edit.  What a plane stage returns points into it and is read by the encoder's label
// stage: it lives to the end of the call.
struct EditScratch {
	DevBuf<uint32_t> erode_p_c_d_keep;         // ckl_erode.hpp's planes P | C | D | K, [nslices][plane_words] each
	DevBuf<uint32_t> dilate_nonzero_gain;      // ckl_dilate.hpp's planes N | gain, [nslices][plane_words] each
	DevBuf<uint64_t> dilate_gain_off;          // [nslices][plane_words]
	DevBuf<uint64_t> dilate_gain_label;        // [gained]
	DevBuf<uint32_t> pool_cut;                 // ckl_downsample.hpp's plane of cuts, [osz][output plane_words]
	DevBuf<uint64_t> pool_cut_off;             // [osz][output plane_words]
	DevBuf<uint64_t> pool_label;               // [cuts]
	// (ckl_combine.hpp's cuts, their offsets and labels stand in the three pool_* buffers: the same triple at the volume's own
	// shape; ckl_crop.hpp's likewise, at the shape of the box whose turn it is)
};

// what the plane stages launch with
struct Road {
	ckl_decoder& d;                    // after its TABLES run (COMBINE: the first stream's)
	ckl_encoder& e;                    // planes_adopt() done: the stages write plane_v / plane_h and d_count_vh [3][ns]
	hipStream_t s;                     // the encode session's
	uint32_t ns;                       // the ENCODER's slices (POOL: not the decoder's)
	dim3 word_grid;                    // a thread per 32-pixel word of the encoder's planes
	unsigned long long* counters;      // zeroed: [0] the largest label, [1] ckl_dilate's, ckl_downsample's, ckl_combine's and ckl_crop's cursor
};

// the decode session's tables as the kernels of this road read them
RunLabels run_labels(const ckl_decoder& d) {
	const RunArrays ra = run_arrays(d);
	RunLabels src;
	src.g = run_geom(d);
	src.word_base = ra.word_base; src.rbase = ra.rbase; src.run_cc = ra.run_cc; src.nruns = ra.nruns;
	src.comp_off = d.d_comp_off.p; src.ncomp = d.d_ncomp_expect.p; src.label_map = d.d_label_map.p;
	return src;
}

// one label per run of session d (src: its tables), at the runs' own bases (in PAINT's scratch of that session), on
// stream s: what erode, dilate, downsample and combine read
const uint64_t* gather_run_labels(ckl_decoder& d, const RunLabels& src, hipStream_t s) {
	d.d_run_label.ensure(d.rtot);
	hipLaunchKernelGGL(k_erode_run_labels, dim3(std::min<uint32_t>((d.max_rcap + kBlock - 1) / kBlock + 1, 256), d.nslices), dim3(kBlock), 0, s, src, d.d_run_label.p);
	return d.d_run_label.p;
}

// The three plane stages.  Each only launches; what the label stage needs beside the tables is what it hands back:
// nothing, the keep plane, the gain triple.
void plain_planes(const Road& r, const RunLabels& src) {
	hipLaunchKernelGGL(k_label_planes_from_runs, r.word_grid, dim3(kBlock), 0, r.s, src, plane_v(r.e), plane_h(r.e, r.ns), r.e.d_count_vh.p, r.ns);
}

// returns the keep plane K; counters[0] takes the largest surviving label
const uint32_t* eroded_planes(const Road& r, const RunLabels& src, const uint64_t* run_label, const LabelEdit& edit, EditScratch& scratch) {
	const size_t pw = r.e.plane_words * r.ns;
	scratch.erode_p_c_d_keep.ensure(4 * pw);
	uint32_t *plane_p = scratch.erode_p_c_d_keep.p, *plane_c = plane_p + pw, *plane_d = plane_c + pw, *keep = plane_d + pw;
	const ErodeArgs ea = { static_cast<uint32_t>(edit.connectivity), edit.keep_border ? 1u : 0u, r.ns };
	hipLaunchKernelGGL(k_erode_terms, r.word_grid, dim3(kBlock), 0, r.s, src, run_label, ea, plane_p, plane_c, plane_d);
	hipLaunchKernelGGL(k_erode_keep, r.word_grid, dim3(kBlock), 0, r.s, src, run_label, ea, plane_p, plane_c, plane_d, keep, r.counters);
	hipLaunchKernelGGL(k_erode_planes, r.word_grid, dim3(kBlock), 0, r.s, src, run_label, keep, plane_v(r.e), plane_h(r.e, r.ns), r.e.d_count_vh.p, r.ns);
	return keep;
}

// returns the number of gained pixels and leaves the gain triple in src; 0: nothing was gained, the triple stays null and
// the planes are the plain ones
unsigned long long dilated_planes(const Road& r, RunLabels& src, const uint64_t* run_label, const LabelEdit& edit, EditScratch& scratch) {
	const size_t pw = r.e.plane_words * r.ns;
	scratch.dilate_nonzero_gain.ensure(2 * pw);
	scratch.dilate_gain_off.ensure(pw);
	uint32_t *plane_n = scratch.dilate_nonzero_gain.p, *gain = plane_n + pw;
	const DilateArgs da = { static_cast<uint32_t>(edit.connectivity), r.ns };
	hipLaunchKernelGGL(k_dilate_nonzero, r.word_grid, dim3(kBlock), 0, r.s, src, run_label, plane_n);
	hipLaunchKernelGGL(k_dilate_gain, r.word_grid, dim3(kBlock), 0, r.s, src.g, da, plane_n, gain, scratch.dilate_gain_off.p, r.counters + 1);
	const unsigned long long gained = download(r.counters + 1, 1, r.s)[0];      // the host sizes the gained pixels' labels
	if (!gained) { plain_planes(r, src); return 0; }
	scratch.dilate_gain_label.ensure(gained);
	hipLaunchKernelGGL(k_dilate_mode, r.word_grid, dim3(kBlock), 0, r.s, src, run_label, da, plane_n, gain, scratch.dilate_gain_off.p, scratch.dilate_gain_label.p);
	src.gain = gain; src.gain_off = scratch.dilate_gain_off.p; src.gain_label = scratch.dilate_gain_label.p;
	hipLaunchKernelGGL(k_dilate_planes, r.word_grid, dim3(kBlock), 0, r.s, src, run_label, plane_v(r.e), plane_h(r.e, r.ns), r.e.d_count_vh.p, r.ns);
	return gained;
}

// Returns the number of cuts and leaves the pooled triple in src; counters[0] takes the largest pooled label.  The word
// grid, the planes and the counts are the pooled volume's, the tables behind src are the input's.
unsigned long long pooled_planes(const Road& r, RunLabels& src, const uint64_t* run_label, const PoolGeom& p, EditScratch& scratch) {
	const size_t pw = p.plane_words * r.ns;
	scratch.pool_cut.ensure(pw);
	scratch.pool_cut_off.ensure(pw);
	hipLaunchKernelGGL(k_pool_cuts, r.word_grid, dim3(kBlock), 0, r.s, src.g, p, scratch.pool_cut.p, scratch.pool_cut_off.p, r.counters + 1);
	const unsigned long long cuts = download(r.counters + 1, 1, r.s)[0];      // the host sizes the pooled runs' labels (every word has a cut: not 0)
	scratch.pool_label.ensure(cuts);
	if (p.fz == 1u) hipLaunchKernelGGL(k_pool_labels<1>, r.word_grid, dim3(kBlock), 0, r.s, src, run_label, p, scratch.pool_cut.p, scratch.pool_cut_off.p, scratch.pool_label.p, r.counters);
	else hipLaunchKernelGGL(k_pool_labels<2>, r.word_grid, dim3(kBlock), 0, r.s, src, run_label, p, scratch.pool_cut.p, scratch.pool_cut_off.p, scratch.pool_label.p, r.counters);
	src.pool_cut = scratch.pool_cut.p; src.pool_off = scratch.pool_cut_off.p; src.pool_label = scratch.pool_label.p;
	src.pool_sx = p.sx; src.pool_sy = p.sy; src.pool_row_words = p.row_words; src.pool_plane_words = p.plane_words;
	hipLaunchKernelGGL(k_pool_planes, r.word_grid, dim3(kBlock), 0, r.s, src, p, plane_v(r.e), plane_h(r.e, r.ns), r.e.d_count_vh.p, r.ns);
	return cuts;
}

// Leaves the combined triple in src (the first stream's tables; the label stage reads the triple alone); counters[0]
// takes the largest combined label.  The two sessions' planes agree in layout (combine() has checked).
void combined_planes(const Road& r, RunLabels& src, const CombineSide& a, const CombineSide& b, int rule, EditScratch& scratch) {
	const size_t pw = r.e.plane_words * r.ns;
	scratch.pool_cut.ensure(pw);
	scratch.pool_cut_off.ensure(pw);
	hipLaunchKernelGGL(k_combine_cuts, r.word_grid, dim3(kBlock), 0, r.s, a.g, b.g, scratch.pool_cut.p, scratch.pool_cut_off.p, r.counters + 1);
	const unsigned long long cuts = download(r.counters + 1, 1, r.s)[0];      // the host sizes the cuts' labels (every word has a cut: not 0)
	scratch.pool_label.ensure(cuts);
	auto* const labels = rule == CKL_COMBINE_OVERLAY ? k_combine_labels<CKL_COMBINE_OVERLAY> : rule == CKL_COMBINE_KEEP_WHERE ? k_combine_labels<CKL_COMBINE_KEEP_WHERE> : k_combine_labels<CKL_COMBINE_DROP_WHERE>;
	hipLaunchKernelGGL(labels, r.word_grid, dim3(kBlock), 0, r.s, a, b, scratch.pool_cut.p, scratch.pool_cut_off.p, scratch.pool_label.p, r.counters);
	src.pool_cut = scratch.pool_cut.p; src.pool_off = scratch.pool_cut_off.p; src.pool_label = scratch.pool_label.p;
	src.pool_sx = a.g.sx; src.pool_sy = a.g.sy; src.pool_row_words = a.g.row_words; src.pool_plane_words = a.g.plane_words;
	const PoolGeom same = { 1u, r.ns, a.g.sx, a.g.sy, a.g.row_words, a.g.plane_words };
	hipLaunchKernelGGL(k_pool_planes, r.word_grid, dim3(kBlock), 0, r.s, src, same, plane_v(r.e), plane_h(r.e, r.ns), r.e.d_count_vh.p, r.ns);
}

// Returns the number of cuts and leaves the box's triple in src (a copy of the session's tables for this box; the label
// stage reads the triple alone); counters[0] takes the largest label of the box.  The word grid, the planes and the counts
// are the box's, the tables behind src are the session's.
unsigned long long cropped_planes(const Road& r, RunLabels& src, const uint64_t* run_label, const CropBox& box, EditScratch& scratch) {
	const PoolGeom& p = box.p;
	const size_t pw = p.plane_words * r.ns;
	scratch.pool_cut.ensure(pw);
	scratch.pool_cut_off.ensure(pw);
	hipLaunchKernelGGL(k_crop_cuts, r.word_grid, dim3(kBlock), 0, r.s, src.g, box, scratch.pool_cut.p, scratch.pool_cut_off.p, r.counters + 1);
	const unsigned long long cuts = download(r.counters + 1, 1, r.s)[0];      // the host sizes the cuts' labels (every word has a cut: not 0)
	scratch.pool_label.ensure(cuts);
	hipLaunchKernelGGL(k_crop_labels, r.word_grid, dim3(kBlock), 0, r.s, src, run_label, box, scratch.pool_cut.p, scratch.pool_cut_off.p, scratch.pool_label.p, r.counters);
	src.pool_cut = scratch.pool_cut.p; src.pool_off = scratch.pool_cut_off.p; src.pool_label = scratch.pool_label.p;
	src.pool_sx = p.sx; src.pool_sy = p.sy; src.pool_row_words = p.row_words; src.pool_plane_words = p.plane_words;
	hipLaunchKernelGGL(k_pool_planes, r.word_grid, dim3(kBlock), 0, r.s, src, p, plane_v(r.e), plane_h(r.e, r.ns), r.e.d_count_vh.p, r.ns);
	return cuts;
}

// lib::pixel_pairs (lib.hpp:249-256): equal neighbours in x-fastest order — inside the rows every pair that V does not
// mark, and the wrap-arounds the plane writer counted.  counts: [3][ns] bits of V | bits of H | wrap pairs
VolumeStats stats_from_counts(const std::vector<uint32_t>& counts, uint64_t max_label, int64_t sx, int64_t sy, uint32_t ns) {
	VolumeStats st;
	st.max_label = max_label;
	for (uint32_t zi = 0; zi < ns; zi++) st.pairs += static_cast<uint64_t>(sx - 1) * sy - counts[zi] + counts[2 * static_cast<size_t>(ns) + zi];
	return st;
}

// the call's line under CKL_PROFILE (tools/*_timing.py and the GPU tests of the six operations read it; CROP: one line per
// box).  extra: DILATE's gained pixels, POOL's, COMBINE's and CROP's pieces
void print_profile(const LabelEdit& edit, double ms_tables, double ms_planes, const ckl_encoder& e, float ms_kernel, unsigned long long extra) {
	double graph = 0, cracks = 0, labels = 0, assembly = 0;
	for (const auto& m : e.host_marks) {
		const std::string name = m.first;
		if (name == "planes" || name == "graph") graph += m.second;
		else if (name == "cracks") cracks += m.second;
		else if (name == "assembly" || name == "codes_d2h") assembly += m.second;
		else labels += m.second;      // f:*, flat, l:*, label_table, labels_d2h: the label side, on the host under the crack trail
	}
	const EditNames& names = kEditNames[edit.kind];
	char tail[40] = "";
	if (edit.kind == LabelEdit::DILATE) snprintf(tail, sizeof(tail), " gained=%llu", extra);
	if (edit.kind == LabelEdit::POOL || edit.kind == LabelEdit::COMBINE || edit.kind == LabelEdit::CROP) snprintf(tail, sizeof(tail), " pieces=%llu", extra);
	fprintf(stderr, "[ckl %s host ms] tables=%.2f %s=%.2f graph=%.2f cracks=%.2f labels=%.2f assembly=%.2f %s=%.3f%s\n",
		names.op, ms_tables, names.planes_field, ms_planes, graph, cracks, labels, assembly, names.device_field, ms_kernel, tail);
}

// What the host refuses, before any device is asked for: the stream's header and the markov order of the output
// (markov_order < 0: the stream's own).
Header checked_header(const uint8_t* buf, uint64_t n, int markov_order, const LabelEdit& edit, uint64_t& order) {
	if (edit.kind == LabelEdit::POOL) {
		if (edit.fx != 2 || edit.fy != 2 || (edit.fz != 1 && edit.fz != 2))
			throw Error(CKL_ERR_ARG, "crackle_amd: downsample: factor must be (2, 2, 1) or (2, 2, 2). Got: (" + std::to_string(edit.fx) + ", " + std::to_string(edit.fy) + ", " + std::to_string(edit.fz) + ")");
	}
	else if ((edit.kind == LabelEdit::ERODE || edit.kind == LabelEdit::DILATE) && edit.connectivity != 6 && edit.connectivity != 18 && edit.connectivity != 26)
		throw Error(CKL_ERR_ARG, std::string("crackle_amd: ") + kEditNames[edit.kind].op + ": connectivity must be 6, 18 or 26. Got: " + std::to_string(edit.connectivity));
	if (n < Header::kBytesV0) throw Error(CKL_ERR_FORMAT, "crackle: Input too small to be a valid stream. Bytes: " + std::to_string(n));
	const Header head = Header::parse(buf, n);
	if (head.is_signed) throw Error(CKL_ERR_ARG, "Signed integer data types are not currently supported.");
	order = markov_order < 0 ? static_cast<uint64_t>(head.markov_model_order) : static_cast<uint64_t>(markov_order);
	if (order > 15) throw Error(CKL_ERR_ARG, "crackle_amd: markov_model_order must be in [0, 15]");
	check_dims(head.sx, head.sy, head.sz, head.data_width, 0);
	return head;
}

// a decode session of the whole stream (or of its slices [z_start, z_end)) after its TABLES run (a damaged slice of the
// session raises here, as for a decode; one outside it is never looked at)
DecoderPtr tables_session(const uint8_t* buf, uint64_t n, int device, int64_t z_start = 0, int64_t z_end = -1) {
	DecoderPtr dec;
	const int rc = open_decoder(buf, n, z_start, z_end, device, dec);
	if (rc != CKL_OK) throw Error(rc, ckl_last_error());
	enter(dec.get());
	decoder_run(*dec, { Goal::TABLES });
	CKL_HIP(hipStreamSynchronize(dec->stream));
	return dec;
}

using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

void recompress(const uint8_t* buf, uint64_t n, int markov_order, int device, const LabelEdit& edit, uint8_t** out, uint64_t* out_len) {
	uint64_t order = 0;
	const Header head = checked_header(buf, n, markov_order, edit, order);
	// the encoder's volume: the decoder's, or the pooled one (an axis of size 0 or 1 keeps its size)
	const bool pool = edit.kind == LabelEdit::POOL;
	const int64_t sx = pool ? (head.sx + 1) / 2 : head.sx, sy = pool ? (head.sy + 1) / 2 : head.sy, sz = pool && edit.fz == 2 ? (head.sz + 1) / 2 : head.sz;
	if (head.voxels() == 0) {
		hand_out(header_bytes(stream_header(head.data_width, sx, sy, sz, VolumeStats(), false, head.fortran_order, order, nullptr)), OutAlloc::MALLOC, out, out_len);
		return;
	}
	select_device(device);      // (what came before needs none: refusals and streams without voxels are the host's)
	const auto t_start = Clock::now();
	const DecoderPtr dec = tables_session(buf, n, device);
	ckl_decoder& d = *dec;
	const auto t_tables = Clock::now();
	RunLabels src = run_labels(d);

	// the planes of the edited labels, in an encode session of this call
	DevBuf<unsigned long long> counters;
	EditScratch scratch;
	ckl_encoder* raw = nullptr;
	if (ckl_encoder_create(sx, sy, sz, head.data_width, device, &raw) != CKL_OK) throw Error(CKL_ERR_RUNTIME, ckl_last_error());
	const EncoderPtr enc(raw);
	ckl_encoder& e = *enc;
	enter(&e);
	const uint32_t ns = static_cast<uint32_t>(sz);
	const uint32_t row_words = static_cast<uint32_t>((sx + 31) / 32);
	const uint64_t plane_words = static_cast<uint64_t>(row_words) * sy;
	planes_adopt(e, row_words, plane_words, ns, 3);
	counters.ensure(2);
	CKL_HIP(hipMemsetAsync(counters.p, 0, 2 * sizeof(unsigned long long), e.stream));
	const Road r = { d, e, e.stream, ns, dim3(static_cast<uint32_t>((plane_words + kBlock - 1) / kBlock), ns), counters.p };
	CKL_HIP(hipEventRecord(e.evd0, r.s));
	const uint64_t* run_label = edit.kind == LabelEdit::NONE ? nullptr : gather_run_labels(d, src, r.s);
	unsigned long long gained = 0;
	if (edit.kind == LabelEdit::ERODE) src.keep = eroded_planes(r, src, run_label, edit, scratch);
	else if (edit.kind == LabelEdit::DILATE) gained = dilated_planes(r, src, run_label, edit, scratch);
	else if (pool) pooled_planes(r, src, run_label, { static_cast<uint32_t>(edit.fz), d.nslices, static_cast<uint32_t>(sx), static_cast<uint32_t>(sy), row_words, plane_words }, scratch);
	else plain_planes(r, src);
	CKL_HIP(hipEventRecord(e.evd1, r.s));
	// (k_erode_keep has taken the largest surviving label, k_pool_labels the largest pooled one; dilation leaves the
	// largest label what it was)
	if (edit.kind != LabelEdit::ERODE && !pool) hipLaunchKernelGGL(k_label_map_max, dim3(static_cast<uint32_t>(std::min<uint64_t>((d.total_comp + kBlock - 1) / kBlock + 1, 1024))), dim3(kBlock), 0, r.s,
		d.d_label_map.p, d.total_comp, counters.p);
	const std::vector<uint32_t> counts = download(e.d_count_vh.p, 3 * static_cast<size_t>(ns), r.s);
	const VolumeStats st = stats_from_counts(counts, download(counters.p, 1, r.s)[0], sx, sy, ns);
	float ms_kernel = 0.f;
	CKL_HIP(hipEventElapsedTime(&ms_kernel, e.evd0, e.evd1));
	const auto t_planes = Clock::now();

	encode_from_planes(e, src, sx, sy, sz, head.data_width, head.fortran_order, order, st, counts, out, out_len);
	// POOL's pieces: the pooled volume's runs, one per row and one more per bit of V (of the cuts, those that changed the label)
	unsigned long long pieces = static_cast<unsigned long long>(sy) * ns;
	for (uint32_t zi = 0; zi < ns; zi++) pieces += counts[zi];
	if (getenv("CKL_PROFILE")) print_profile(edit, ms_between(t_start, t_tables), ms_between(t_tables, t_planes), e, ms_kernel, pool ? pieces : gained);
}

// what the kernels of ckl_combine.hpp read of session d: its tables and one label per run, gathered on stream s
CombineSide combine_side(ckl_decoder& d, hipStream_t s) {
	const RunLabels t = run_labels(d);
	return { t.g, t.word_base, t.rbase, t.nruns, gather_run_labels(d, t, s) };
}

const char* combine_name(int rule) { return rule == CKL_COMBINE_OVERLAY ? "overlay" : "mask_by"; }

// recompress()'s sibling for two streams of one shape: the same road from the plane stage on, with two decode sessions,
// a then b, alive to its end.  The output's data width is a's, for CKL_COMBINE_OVERLAY the larger of the two.
void combine(const uint8_t* buf_a, uint64_t n_a, const uint8_t* buf_b, uint64_t n_b, int rule, int markov_order, int device, uint8_t** out, uint64_t* out_len) {
	LabelEdit edit;
	edit.kind = LabelEdit::COMBINE; edit.rule = rule;
	if (rule != CKL_COMBINE_OVERLAY && rule != CKL_COMBINE_KEEP_WHERE && rule != CKL_COMBINE_DROP_WHERE)
		throw Error(CKL_ERR_ARG, "crackle_amd: combine: unknown rule: " + std::to_string(rule));
	if (n_a < Header::kBytesV0 || n_b < Header::kBytesV0) throw Error(CKL_ERR_FORMAT, "crackle: Input too small to be a valid stream. Bytes: " + std::to_string(n_a < Header::kBytesV0 ? n_a : n_b));
	const Header shape_a = Header::parse(buf_a, n_a), shape_b = Header::parse(buf_b, n_b);
	if (shape_a.sx != shape_b.sx || shape_a.sy != shape_b.sy || shape_a.sz != shape_b.sz)
		throw Error(CKL_ERR_ARG, std::string("crackle_amd: ") + combine_name(rule) + ": the volumes differ in shape: " + std::to_string(shape_a.sx) + " x " + std::to_string(shape_a.sy) + " x " + std::to_string(shape_a.sz)
			+ " and " + std::to_string(shape_b.sx) + " x " + std::to_string(shape_b.sy) + " x " + std::to_string(shape_b.sz));
	uint64_t order = 0, order_b = 0;
	const Header head = checked_header(buf_a, n_a, markov_order, edit, order);
	const Header head_b = checked_header(buf_b, n_b, 0, edit, order_b);      // (the order is a's or the caller's)
	const int data_width = rule == CKL_COMBINE_OVERLAY ? std::max(head.data_width, head_b.data_width) : head.data_width;
	const int64_t sx = head.sx, sy = head.sy, sz = head.sz;
	if (head.voxels() == 0) {
		hand_out(header_bytes(stream_header(data_width, sx, sy, sz, VolumeStats(), false, head.fortran_order, order, nullptr)), OutAlloc::MALLOC, out, out_len);
		return;
	}
	select_device(device);      // (what came before needs none: refusals and streams without voxels are the host's)
	const auto t_start = Clock::now();
	const DecoderPtr dec_a = tables_session(buf_a, n_a, device);      // (a damaged slice of a raises before b is looked at)
	const DecoderPtr dec_b = tables_session(buf_b, n_b, device);
	const auto t_tables = Clock::now();
	RunLabels src = run_labels(*dec_a);
	const RunGeom gb = run_geom(*dec_b);
	if (src.g.sx != gb.sx || src.g.sy != gb.sy || src.g.row_words != gb.row_words || src.g.plane_words != gb.plane_words || dec_a->nslices != dec_b->nslices)
		throw Error(CKL_ERR_RUNTIME, std::string("crackle_amd: ") + combine_name(rule) + ": the sessions' crack planes differ in layout");

	DevBuf<unsigned long long> counters;
	EditScratch scratch;
	ckl_encoder* raw = nullptr;
	if (ckl_encoder_create(sx, sy, sz, data_width, device, &raw) != CKL_OK) throw Error(CKL_ERR_RUNTIME, ckl_last_error());
	const EncoderPtr enc(raw);
	ckl_encoder& e = *enc;
	enter(&e);
	const uint32_t ns = static_cast<uint32_t>(sz);
	const uint32_t row_words = static_cast<uint32_t>((sx + 31) / 32);
	const uint64_t plane_words = static_cast<uint64_t>(row_words) * sy;
	if (row_words != src.g.row_words || plane_words != src.g.plane_words || ns != dec_a->nslices)
		throw Error(CKL_ERR_RUNTIME, std::string("crackle_amd: ") + combine_name(rule) + ": the session's crack planes are not the volume's");
	planes_adopt(e, row_words, plane_words, ns, 3);
	counters.ensure(2);
	CKL_HIP(hipMemsetAsync(counters.p, 0, 2 * sizeof(unsigned long long), e.stream));
	const Road r = { *dec_a, e, e.stream, ns, dim3(static_cast<uint32_t>((plane_words + kBlock - 1) / kBlock), ns), counters.p };
	CKL_HIP(hipEventRecord(e.evd0, r.s));
	const CombineSide side_a = combine_side(*dec_a, r.s), side_b = combine_side(*dec_b, r.s);
	combined_planes(r, src, side_a, side_b, rule, scratch);
	CKL_HIP(hipEventRecord(e.evd1, r.s));
	const std::vector<uint32_t> counts = download(e.d_count_vh.p, 3 * static_cast<size_t>(ns), r.s);
	const VolumeStats st = stats_from_counts(counts, download(counters.p, 1, r.s)[0], sx, sy, ns);      // (k_combine_labels has taken the largest combined label)
	float ms_kernel = 0.f;
	CKL_HIP(hipEventElapsedTime(&ms_kernel, e.evd0, e.evd1));
	const auto t_planes = Clock::now();

	encode_from_planes(e, src, sx, sy, sz, data_width, head.fortran_order, order, st, counts, out, out_len);
	// the combined volume's runs, counted as POOL counts its pieces: one per row and one more per bit of V
	unsigned long long pieces = static_cast<unsigned long long>(sy) * ns;
	for (uint32_t zi = 0; zi < ns; zi++) pieces += counts[zi];
	if (getenv("CKL_PROFILE")) print_profile(edit, ms_between(t_start, t_tables), ms_between(t_tables, t_planes), e, ms_kernel, pieces);
}

// a box of a crop call: [x0, x1) x [y0, y1) x [z0, z1) of the stream's volume
struct Box {
	int64_t x0, x1, y0, y1, z0, z1;
	int64_t wx() const { return x1 - x0; }
	int64_t wy() const { return y1 - y0; }
	int64_t wz() const { return z1 - z0; }
	bool empty() const { return wx() == 0 || wy() == 0 || wz() == 0; }
};

// recompress()'s sibling for many outputs: one stream per box, each the stream compress() gives for the box's voxels.
// One decode session over the z-range that the boxes with voxels span, one TABLES run and one label per run for all of
// them; then a turn per box through ckl_crop.hpp's kernels and the encoder.  Boxes of one shape share an encode session.
// outs / out_lens: n_boxes entries, null / 0 on entry; whoever calls frees what stands there when this throws.
void crop_boxes(const uint8_t* buf, uint64_t n, const Box* boxes, uint64_t n_boxes, int markov_order, int device, uint8_t** outs, uint64_t* out_lens) {
	LabelEdit edit;
	edit.kind = LabelEdit::CROP;
	uint64_t order = 0;
	const Header head = checked_header(buf, n, markov_order, edit, order);
	// every box is checked before any device work
	for (uint64_t k = 0; k < n_boxes; k++) {
		check_box_axis("crop", "x", boxes[k].x0, boxes[k].x1, head.sx);
		check_box_axis("crop", "y", boxes[k].y0, boxes[k].y1, head.sy);
		check_box_axis("crop", "z", boxes[k].z0, boxes[k].z1, head.sz);
	}
	// boxes without voxels are the host's: the header-only stream of their shape
	int64_t zmin = INT64_MAX, zmax = -1;
	for (uint64_t k = 0; k < n_boxes; k++) {
		const Box& b = boxes[k];
		if (b.empty()) hand_out(header_bytes(stream_header(head.data_width, b.wx(), b.wy(), b.wz(), VolumeStats(), false, head.fortran_order, order, nullptr)), OutAlloc::MALLOC, outs + k, out_lens + k);
		else { zmin = std::min(zmin, b.z0); zmax = std::max(zmax, b.z1); }
	}
	if (zmax < 0) return;
	select_device(device);      // (what came before needs none)
	const auto t_start = Clock::now();
	const DecoderPtr dec = tables_session(buf, n, device, zmin, zmax);      // (a damaged slice of [zmin, zmax) raises here, whichever box is asked for)
	ckl_decoder& d = *dec;
	if (d.nslices != static_cast<uint32_t>(zmax - zmin)) throw Error(CKL_ERR_RUNTIME, "crackle_amd: crop: the session's slices are not the boxes' z-range");
	const RunLabels tables = run_labels(d);
	const uint64_t* run_label = gather_run_labels(d, tables, d.stream);
	CKL_HIP(hipStreamSynchronize(d.stream));      // (the encode sessions' streams do not wait for the decoder's)
	double ms_tables = ms_between(t_start, Clock::now());

	DevBuf<unsigned long long> counters;
	counters.ensure(2);
	EditScratch scratch;
	std::map<std::tuple<int64_t, int64_t, int64_t>, EncoderPtr> sessions;      // one per shape of box
	for (uint64_t k = 0; k < n_boxes; k++) {
		const Box& b = boxes[k];
		if (b.empty()) continue;
		const auto t_box = Clock::now();
		const int64_t sx = b.wx(), sy = b.wy(), sz = b.wz();
		EncoderPtr& enc = sessions[std::make_tuple(sx, sy, sz)];
		if (!enc) {
			ckl_encoder* raw = nullptr;
			if (ckl_encoder_create(sx, sy, sz, head.data_width, device, &raw) != CKL_OK) throw Error(CKL_ERR_RUNTIME, ckl_last_error());
			enc.reset(raw);
		}
		ckl_encoder& e = *enc;
		enter(&e);
		const uint32_t ns = static_cast<uint32_t>(sz);
		const uint32_t row_words = static_cast<uint32_t>((sx + 31) / 32);
		const uint64_t plane_words = static_cast<uint64_t>(row_words) * sy;
		planes_adopt(e, row_words, plane_words, ns, 3);
		CKL_HIP(hipMemsetAsync(counters.p, 0, 2 * sizeof(unsigned long long), e.stream));
		const Road r = { d, e, e.stream, ns, dim3(static_cast<uint32_t>((plane_words + kBlock - 1) / kBlock), ns), counters.p };
		const CropBox box = { static_cast<uint32_t>(b.x0), static_cast<uint32_t>(b.y0), static_cast<uint32_t>(b.z0 - zmin),
			{ 1u, ns, static_cast<uint32_t>(sx), static_cast<uint32_t>(sy), row_words, plane_words } };
		RunLabels src = tables;
		CKL_HIP(hipEventRecord(e.evd0, r.s));
		cropped_planes(r, src, run_label, box, scratch);
		CKL_HIP(hipEventRecord(e.evd1, r.s));
		const std::vector<uint32_t> counts = download(e.d_count_vh.p, 3 * static_cast<size_t>(ns), r.s);
		const VolumeStats st = stats_from_counts(counts, download(counters.p, 1, r.s)[0], sx, sy, ns);      // (k_crop_labels has taken the box's largest label)
		float ms_kernel = 0.f;
		CKL_HIP(hipEventElapsedTime(&ms_kernel, e.evd0, e.evd1));
		const auto t_planes = Clock::now();

		encode_from_planes(e, src, sx, sy, sz, head.data_width, head.fortran_order, order, st, counts, outs + k, out_lens + k);
		// the box's runs, counted as POOL and COMBINE count their pieces: one per row and one more per bit of V
		unsigned long long pieces = static_cast<unsigned long long>(sy) * ns;
		for (uint32_t zi = 0; zi < ns; zi++) pieces += counts[zi];
		if (getenv("CKL_PROFILE")) print_profile(edit, ms_tables, ms_between(t_box, t_planes), e, ms_kernel, pieces);
		ms_tables = 0;      // (the shared run stands on the first box's line)
	}
}

// the C entry of crop_boxes: boxes as [n_boxes][6] x0 x1 y0 y1 z0 z1; on any error every stream already handed out is
// freed and all of outs are left null
void crop_entry(const uint8_t* buf, uint64_t n, const int64_t* boxes, uint64_t n_boxes, int flags, int markov_order, int device, uint8_t** outs, uint64_t* out_lens) {
	if (flags) throw Error(CKL_ERR_ARG, "crackle_amd: crop: flags must be 0");
	if (n_boxes == 0) return;
	if (!buf || !boxes || !outs || !out_lens) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
	std::vector<Box> bx(n_boxes);
	for (uint64_t k = 0; k < n_boxes; k++) {
		bx[k] = { boxes[6 * k], boxes[6 * k + 1], boxes[6 * k + 2], boxes[6 * k + 3], boxes[6 * k + 4], boxes[6 * k + 5] };
		outs[k] = nullptr; out_lens[k] = 0;
	}
	try {
		crop_boxes(buf, n, bx.data(), n_boxes, markov_order, device, outs, out_lens);
	}
	catch (...) {
		for (uint64_t k = 0; k < n_boxes; k++) {
			if (outs[k]) ckl_free(outs[k]);
			outs[k] = nullptr; out_lens[k] = 0;
		}
		throw;
	}
}

}  // namespace

extern "C" {

int ckl_recompress(const uint8_t* buf, uint64_t n, int markov_model_order, int device, uint8_t** out, uint64_t* out_len) {
	return guard([&] {
		if (!buf || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		recompress(buf, n, markov_model_order, device, LabelEdit(), out, out_len);
	});
}

int ckl_erode(const uint8_t* buf, uint64_t n, int connectivity, int flags, int markov_model_order, int device, uint8_t** out, uint64_t* out_len) {
	return guard([&] {
		if (!buf || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		if (flags & ~CKL_ERODE_KEEP_BORDER) throw Error(CKL_ERR_ARG, "crackle_amd: erode: unknown flags");
		recompress(buf, n, markov_model_order, device, { LabelEdit::ERODE, connectivity, (flags & CKL_ERODE_KEEP_BORDER) != 0 }, out, out_len);
	});
}

int ckl_dilate(const uint8_t* buf, uint64_t n, int connectivity, int flags, int markov_model_order, int device, uint8_t** out, uint64_t* out_len) {
	return guard([&] {
		if (!buf || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		if (flags) throw Error(CKL_ERR_ARG, "crackle_amd: dilate: flags must be 0");
		recompress(buf, n, markov_model_order, device, { LabelEdit::DILATE, connectivity, false }, out, out_len);
	});
}

int ckl_downsample(const uint8_t* buf, uint64_t n, int fx, int fy, int fz, int flags, int markov_model_order, int device, uint8_t** out, uint64_t* out_len) {
	return guard([&] {
		if (!buf || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		if (flags) throw Error(CKL_ERR_ARG, "crackle_amd: downsample: flags must be 0");
		LabelEdit edit;
		edit.kind = LabelEdit::POOL; edit.fx = fx; edit.fy = fy; edit.fz = fz;
		recompress(buf, n, markov_model_order, device, edit, out, out_len);
	});
}

int ckl_combine(const uint8_t* buf_a, uint64_t n_a, const uint8_t* buf_b, uint64_t n_b, int rule, int flags, int markov_model_order, int device, uint8_t** out, uint64_t* out_len) {
	return guard([&] {
		if (!buf_a || !buf_b || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		if (flags) throw Error(CKL_ERR_ARG, "crackle_amd: combine: flags must be 0");
		combine(buf_a, n_a, buf_b, n_b, rule, markov_model_order, device, out, out_len);
	});
}

int ckl_crop_boxes(const uint8_t* buf, uint64_t n, const int64_t* boxes, uint64_t n_boxes, int flags, int markov_model_order, int device, uint8_t** outs, uint64_t* out_lens) {
	return guard([&] { crop_entry(buf, n, boxes, n_boxes, flags, markov_model_order, device, outs, out_lens); });
}

int ckl_crop(
	const uint8_t* buf, uint64_t n, int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1,
	int flags, int markov_model_order, int device, uint8_t** out, uint64_t* out_len
) {
	const int64_t box[6] = { x0, x1, y0, y1, z0, z1 };
	return ckl_crop_boxes(buf, n, box, 1, flags, markov_model_order, device, out, out_len);
}

}  // extern "C"
