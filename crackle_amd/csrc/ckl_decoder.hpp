// The decode session (built and run by ckl_decode.hip) and what the operations on a decoded stream
// (ckl_operations.hip) need of it: a consumer asks decoder_run for a goal (RunRequest), builds its
// kernels' argument blocks with run_geom / run_arrays and launches on the session's stream.
#pragma once

#include "ckl_common.hpp"
#include "ckl_run_types.hpp"

#include <memory>

namespace ckl {

// k_run_stats' arguments (ckl_operations.hip); the pipeline launches it for Goal::STATS
struct StatsArgs {
	const uint64_t* table;     // label values as label_map holds them (sign-extended), ascending as unsigned
	uint32_t n_table;
	unsigned long long* acc;   // [n_table][4]: N, sum x, sum y, sum z
	uint32_t* box;             // [n_table][6]: xmin ymin zmin xmax ymax zmax
	uint32_t sx, n_pixels;
	uint32_t z_start;
	uint32_t lds_comps;        // per-component accumulators the workgroup's LDS holds
};

constexpr int kMaxStages = 20;

}  // namespace ckl

struct ckl_decoder {
	using Header = ckl::Header;
	template <typename T> using DevBuf = ckl::DevBuf<T>;
	static constexpr int kMaxStages = ckl::kMaxStages;

	int device = 0;
	int n_cus = 256;
	int max_lds = 0;
	hipStream_t stream = nullptr;
	// stage boundaries: ev[i] .. ev[i+1] brackets stage i of the last run
	hipEvent_t ev[kMaxStages + 2] = {};      // [kMaxStages + 1]: end of the pipeline
	hipEvent_t ev_in = nullptr;
	const char* stage_name[kMaxStages] = {};
	float stage_ms[kMaxStages] = {};
	int n_stages = 0;
	float pipeline_ms = 0.f;

	Header head;
	uint64_t n_bytes = 0;
	int64_t z_start = 0, z_end = 0;
	uint32_t nslices = 0;
	uint64_t sxy = 0;

	// device residents
	DevBuf<uint8_t> d_stream;            // the whole stream (a view of the caller's buffer for ckl_decoder_create_device)
	DevBuf<uint8_t> d_desc;              // the per-slice descriptor tables, one block, one upload
	void* desc_staging = nullptr;        // pinned host image of d_desc (host_out_alloc), kept until the session dies
	uint32_t* host_flags = nullptr;      // pinned: the runs' per-slice error words + overflow word land here
	bool host_flags_pinned = false;
	bool flags_by_resolve = false;       // this run: k_slice_resolve wrote them there itself (ResolveArgs::host_flags)
	bool stage_events = true;            // HIP events between the kernels (ckl_decoder_stage_timing); off: only around the pipeline
	bool pending_upload = false;         // decoder_build left copies in flight that no run has waited for yet (ckl_decoder_destroy waits)
	bool stream_resident = false;        // the stream was in HBM already: capacities come from the z-index alone
	DevBuf<uint64_t> d_code_off, d_cbase, d_nbase, d_comp_off, d_rbase;
	DevBuf<uint32_t> d_code_len, d_ccap, d_ncap, d_rcap;
	DevBuf<uint8_t> d_model, d_ctl_kind;
	DevBuf<uint32_t> d_symbuf;
	DevBuf<uint64_t> d_symbase;
	DevBuf<uint32_t> d_mkscratch;
	DevBuf<uint64_t> d_mkbase;
	DevBuf<uint32_t> d_upacked, d_ctl_dx, d_ctl_dy, d_ctl_lastT, d_seg_x, d_seg_y, d_nodes;
	DevBuf<int32_t> d_ctl_depth, d_ctl_gmin;
	DevBuf<unsigned long long> d_ctl_link;
	uint32_t lds_controls = 0;          // capacity of k_decode_cracks' LDS control tables
	size_t lds_bytes = 0;               // dynamic LDS of k_decode_cracks: the tables, or everything the workgroup may have (raster bands)
	DevBuf<uint32_t> d_planes;          // V then H
	DevBuf<uint32_t> d_word_base, d_parent, d_run_start, d_run_cc, d_nruns, d_ncomp, d_ncomp_expect, d_blk_roots;
	DevBuf<uint16_t> d_run_local;
	DevBuf<uint64_t> d_run_label;       // typed on use (1..8 bytes per run)
	DevBuf<uint64_t> d_stats_table;     // ckl_decoder_label_stats: sorted label values
	DevBuf<unsigned long long> d_stats_acc;
	DevBuf<uint32_t> d_stats_box;
	std::vector<uint64_t> stats_table;
	bool bg_unlisted = false;           // pin stream whose background colour is not in its unique list
	std::shared_ptr<DevBuf<uint32_t>> G;      // geometric-sum table of the slice size, shared by the sessions of a device (geom_table)
	DevBuf<uint32_t> d_crc_acc, d_crc_expect, d_slice_err;
	DevBuf<uint64_t> d_label_map;
	DevBuf<uint64_t> d_pin_index, d_pin_depth, d_pin_label, d_pin_work_off, d_ccl_id, d_ccl_label;
	// strip path (ckl_strips.hpp): one slot of strip_cap entries per strip
	DevBuf<uint32_t> d_strip_nruns, d_strip_nsc, d_overflow, d_sc_w, d_sc_cc;
	DevBuf<uint16_t> d_seam_first, d_seam_last, d_row_run, d_run_lid;
	DevBuf<uint64_t> d_sc_label;        // typed on use
	DevBuf<unsigned long long> d_diag;
	bool strip_ok = false;              // shape / layout qualify for the strip path
	// crack records (ckl_crack_records.hpp): the strip path's front end
	bool use_records = false;           // k_crack_records + rasterising strip kernel instead of k_decode_cracks
	uint32_t resolve_cap = 12288;       // strip components of a slice k_slice_resolve's table holds (dynamic LDS)
	uint32_t resolve_cap_max = 12288;   // with a CU's LDS to itself: a run whose slices overflow resolve_cap is repeated with this one before the general pipeline is asked
	DevBuf<uint4> d_rec;
	DevBuf<uint32_t> d_rec_count;
	DevBuf<uint4> d_words;             // WordRec per word of 16 code positions, parked between the two passes of k_crack_match
	DevBuf<uint64_t> d_word_off;
	uint32_t max_words = 0;             // most words of one slice
	uint32_t rec_cap = 0, rec_lds_controls = 0;
	int rec_block = 0;                  // threads of k_crack_match's workgroups: kRecBlock (decoder_new) or kRecBlockWide (decoder_build)
	size_t rec_lds = 0;
	const uint64_t* foreign_label_map = nullptr;   // array_equal: component -> label table of ANOTHER stream (same component counts)
	int paint_width = 0;                // array_equal: bytes per painted voxel when it is not this stream's data width
	std::vector<uint32_t> ncomp_expect_host;       // components per slice of the range, as the label section states them
	bool use_general = false;           // a run overflowed the strip path's LDS tables: stay on the general pipeline
	uint32_t strip_rows = 0, nstrips = 0, strip_cap = 0;
	uint64_t rtot = 0;                  // entries of the general pipeline's per-run arrays (allocated when it runs)
	static constexpr int kMaxChunks = 8;
	hipStream_t chunk_stream[kMaxChunks] = {};
	hipEvent_t chunk_done[kMaxChunks] = {};
	hipEvent_t ev_fork = nullptr;

	// label section layout
	uint64_t total_comp = 0;            // components in [z_start, z_end)
	uint64_t comp_left = 0;             // global id of the first component of z_start
	uint64_t keys_offset = 0, uniq_offset = 0, num_unique = 0;
	int key_width = 1;
	uint64_t bgcolor = 0;
	uint64_t n_pins = 0, pin_total_work = 0, n_ccl = 0;

	uint32_t row_words = 0;
	uint64_t plane_words = 0;
	uint32_t max_rcap = 0;
	uint32_t max_comp = 1;              // most components of one slice in the range
	uint32_t idbits = 1, crc_fix = 0;
	bool check_crc = true;

	~ckl_decoder() {
		for (auto& e : ev) if (e) (void)hipEventDestroy(e);
		if (ev_in) (void)hipEventDestroy(ev_in);
		if (ev_fork) (void)hipEventDestroy(ev_fork);
		for (auto& e : chunk_done) if (e) (void)hipEventDestroy(e);
		for (auto& cs : chunk_stream) if (cs) (void)hipStreamDestroy(cs);
		if (stream) (void)hipStreamDestroy(stream);
		if (desc_staging) ckl::host_out_free(desc_staging);
		if (host_flags) ckl::host_out_free(host_flags);
	}
};

namespace ckl {

// a stored label value, sign-extended as label_map holds it
inline uint64_t read_stored(const Header& h, const uint8_t* lb, uint64_t offset) {
	const int w = h.stored_data_width;
	uint64_t v = rd_le(lb + offset, w);
	if (h.is_signed && w < 8 && (v >> (8 * w - 1))) v |= ~0ull << (8 * w);
	return v;
}

struct StageTimer {
	ckl_decoder& d;
	hipStream_t s;
	int i = 0;
	bool on = true;      // off: z-chunks overlap on several streams, only the whole pipeline is timed
	StageTimer(ckl_decoder& dec, hipStream_t st) : d(dec), s(st) { on = dec.stage_events; CKL_HIP(hipEventRecord(d.ev[0], s)); }
	void done(const char* name) {
		if (!on || i >= kMaxStages) return;
		d.stage_name[i] = name;
		CKL_HIP(hipEventRecord(d.ev[i + 1], s));
		i++;
	}
};

// How far a run of the pipeline (ckl_decode.hip) goes.  Every goal includes the ones before it,
// except that PAINT on the strip path never builds the run tables.
enum class Goal {
	PLANES,      // the crack planes
	TABLES,      // + run tables, component ids, component -> label map, k_check
	STATS,       // + k_run_stats
	PAINT,       // the labels
};

struct RunRequest {
	Goal goal = Goal::PAINT;
	void* out = nullptr;               // PAINT: device buffer of `capacity` bytes
	uint64_t capacity = 0;
	int has_label = 0;                 // PAINT: one byte per voxel, 1 where the voxel's label is `label`
	uint64_t label = 0;
	const StatsArgs* stats = nullptr;  // STATS
	uint32_t* verdicts = nullptr;      // [nslices]: the slices' error words are reported here and nothing is raised for them
	bool x_fastest = false;            // PAINT: x fastest whatever the stream's fortran_order (the encoder's input layout: ckl_paste)
};

// a call on a session begins: its device current, its stream behind the caller's default stream
inline void enter(ckl_decoder* d) {
	if (!d) throw Error(CKL_ERR_ARG, "crackle_amd: null decoder");
	select_device(d->device);
	wait_for_default_stream(d->stream, d->ev_in);
}

// The only entry to the pipeline.  A slice that fails its checks raises slice_error (unless the
// request wants the verdicts); the strip path's overflows are retried here with the same request.
void decoder_run(ckl_decoder& d, const RunRequest& rq);
// the exception for error word `e` (not 0) of slice zi of the range
Error slice_error(const ckl_decoder& d, uint32_t zi, uint32_t e);
// the kernels' views of the session's planes and run tables (there after TABLES / STATS)
dev::RunGeom run_geom(const ckl_decoder& d);
dev::RunArrays run_arrays(const ckl_decoder& d);
// Goal::STATS: k_run_stats on the session's stream (ckl_operations.hip)
void launch_run_stats(ckl_decoder& d, const dev::RunArrays& ra, const StatsArgs& sa);
// the box [x0, x1) x [y0, y1) of the session's slices, dense, into a device buffer: a TABLES run, then
// k_paint_window (ckl_operations.hip); bounds outside the slice and a buffer too small are CKL_ERR_ARG
void decoder_cutout(ckl_decoder& d, int64_t x0, int64_t x1, int64_t y0, int64_t y1, void* out_device, uint64_t capacity, int has_label, uint64_t label);
// 0 <= a <= b <= dim for operation `what` (cutout, paste), or CKL_ERR_ARG naming the axis: nothing is clamped
// (check_bounds, crackle/array.py:529-532)
inline void check_box_axis(const char* what, const char* axis, int64_t a, int64_t b, uint32_t dim) {
	if (a < 0 || a > b || b > static_cast<int64_t>(dim))
		throw Error(CKL_ERR_ARG, std::string("crackle_amd: ") + what + ": " + axis + " range " + std::to_string(a) + " - " + std::to_string(b) + " is not an ascending range inside 0 - " + std::to_string(dim));
}

}  // namespace ckl
