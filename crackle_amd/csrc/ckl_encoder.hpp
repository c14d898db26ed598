// The encode session (created and run by ckl_encode.hip) and what the flat label stage (ckl_encode_labels.hip), the pin
// stage (ckl_encode_pins.hip) and the road from a decode session's tables (ckl_recompress.hip) need of it: the session's
// streams and scratch, the label stage's own part of it (LabelStage), the small transfers, the host timer, enter(), and
// that road's door (planes_adopt, encode_from_planes).
#pragma once

#include "ckl_common.hpp"

#include <chrono>
#include <utility>

struct VolumeStats { uint64_t max_label = 0, pairs = 0, first = 0, last = 0; };
namespace ckl { namespace dev { struct RunLabels; } }

// What the flat label stage keeps in the session and nobody else names (ckl_encode_labels.hip).  What the stage leaves
// for others (d_mapping, d_labels_bin, d_slice_err2) stands in the session itself.
struct LabelStage {
	template <typename T> using DevBuf = ckl::DevBuf<T>;

	// run-based CCL (ckl_runs.hpp)
	DevBuf<uint64_t> d_rbase, d_comp_off;
	DevBuf<uint32_t> d_rcap, d_word_base, d_parent, d_run_start, d_run_cc, d_comp_pix, d_nruns, d_ncomp, d_idbits, d_blk_roots;
	DevBuf<uint16_t> d_run_local;
	DevBuf<uint32_t> d_G, d_crc_acc;
	DevBuf<uint32_t> d_flat_report;     // [4][nslices] + 1: ncomp | crc_acc | idbits | slice_err2 (views: the three above and the session's d_slice_err2) | the strip kernels' overflow word
	uint64_t g_table_pixels = 0;                // slice size the G table was built for
	DevBuf<uint64_t> d_sorted, d_uniq, d_label_hash, d_label_list;      // the label table (flat_section)
	DevBuf<uint32_t> d_n_uniq, d_uniq_blk;
	std::vector<uint64_t> h_rbase;
	std::vector<uint32_t> h_rcap;
	std::vector<uint64_t> h_comp_off;  // first component of every slice: stays alive while its upload is in flight
	// flat labels from the strip kernels (ckl_strips.hpp; flat_enqueue / flat_collect): per-strip tables, then the labels
	// of every slice's components in a slot of flat_resolve_cap entries
	DevBuf<uint16_t> s_run_lid, s_seam_first, s_seam_last;
	DevBuf<uint32_t> s_sc_w, s_sc_first, s_strip_nruns, s_strip_nsc;
	DevBuf<uint64_t> d_label_slots;
	uint32_t flat_nstrips = 0, flat_strip_rows = 0, flat_strip_cap = 0, flat_resolve_cap = 0;
	int max_lds = 0;                   // the device's LDS per workgroup (asked once)
	bool flat_strips = false;          // the label stage that is enqueued runs on the strip kernels
};

struct ckl_encoder {
	template <typename T> using DevBuf = ckl::DevBuf<T>;

	int device = 0;
	hipStream_t stream = nullptr;      // crack codes
	hipStream_t stream2 = nullptr;     // labels (components, crcs, label table), concurrent with the crack trail
	hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_in = nullptr;
	hipEvent_t evd0 = nullptr, evd1 = nullptr;      // around k_trail_walk
	hipEvent_t ev_prezero = nullptr;   // trail_prezero()'s fills on stream2 are done
	float pipeline_ms = 0.f, dominant_ms = 0.f;
	int dtype_bytes = 0;

	DevBuf<unsigned long long> d_stats;
	DevBuf<uint4> d_adjm;                        // crack graph in micro-tiles (ckl_trail.hpp)
	DevBuf<uint32_t> d_slice_err;
	DevBuf<uint64_t> d_cbase, d_sbase, d_kbase, d_pbase, d_bbase, d_out_off;
	DevBuf<uint32_t> d_ccap, d_scap, d_kcap;
	DevBuf<uint8_t> d_crack_tables;               // packed block behind the per-slice base / capacity tables of crack_pass
	DevBuf<uint8_t> d_cp, d_fcode, d_dcode, d_payload, d_boc, d_codes_out, d_model;
	DevBuf<uint32_t> d_code_report;
	uint64_t codes_capacity = 0;        // bound of all slices' BOC + payload bytes
	bool defer_codes = false;           // ckl_encoder_defer_codes: the codes stay in d_codes_out for ckl_encoder_codes_to_host
	bool keep_device_stream = false;    // ckl_encoder_keep_device_stream: every run also assembles the whole stream in HBM
	bool async_host_copy = false;       // ckl_encoder_async_host_copy: a run returns when the stream is complete in HBM; its crack codes reach the host buffer on stream_copy
	bool host_copy_pending = false;     // ... until ckl_encoder_host_wait
	hipStream_t stream_copy = nullptr;
	hipStream_t stream_tab = nullptr;   // the pin stage's label lists come to the host beside the passes of the label stream
	hipEvent_t ev_codes = nullptr;
	void* tables_staging = nullptr;              // pinned host image of d_crack_tables (crack_pass: UploadPacker::commit)
	bool uploads_by_kernel = false;              // this run's small uploads go by upload_small's kernel (flat label streams)
	hipEvent_t ev_labels_crc = nullptr;          // the label section's crc32c stands in d_labels_crc (device-resident streams: ckl_encoder_run)
	DevBuf<uint32_t> d_labels_crc;               // [0]: the crc, [1 ..]: the workgroups' states
	DevBuf<uint8_t> d_stream_out;       // ... here (valid until the next run)
	uint64_t device_stream_bytes = 0;
	uint64_t last_codes_total = 0;      // bytes of the last run's crack codes
	DevBuf<uint32_t> d_stack_node, d_stack_code;
	DevBuf<uint32_t> d_chain_node, d_chain_off, d_chain_clen, d_chain_order, d_chain_dst, d_chain_vstart;
	DevBuf<uint32_t> d_n_chains, d_n_raw, d_n_valid, d_payload_len, d_boc_len;
	DevBuf<uint32_t> d_hist;
	// label planes
	DevBuf<uint32_t> d_planes, d_count_vh;
	uint32_t row_words = 0;
	uint64_t plane_words = 0;
	std::vector<uint32_t> count_v, count_h;     // differing neighbour pairs per slice (host copy)
	LabelStage ls;                               // the flat label stage's own tables and plan (ckl_encode_labels.hip)
	DevBuf<uint64_t> d_mapping;                  // the label of every component, slice after slice (flat_collect, the pin stage)
	DevBuf<uint32_t> d_cc_volume;                // global component id of every voxel (pin encoding only)
	DevBuf<uint32_t> d_pin_kept, d_pin_u32;      // pin passes (ckl_pins_dev.hpp): kept-run marks (uint16 per voxel), per-component depths
	DevBuf<uint8_t> d_pin_tables;                // per-row label tables of k_pin_dedup
	DevBuf<uint64_t> d_pin_u64;                  // per-component keys
	DevBuf<uint32_t> d_slice_err2;               // the label stage's error word per slice (a view of its report), the pin stage's error word
	DevBuf<uint8_t> d_labels_bin;                // the flat label section, assembled on device
	// label planes left by ckl_encoder_stats for the ckl_encoder_run that follows on the same
	// volume (the sharded encoder: stats -> all-gather -> run with the agreed formats)
	const void* planes_for = nullptr;
	// ckl_encoder_markov_stats leaves the whole trail behind (difference codes, chains, BOC index): the run that
	// follows for the same volume and crack format only packs them under the agreed model (single use, like the planes)
	const void* trail_for = nullptr;
	bool trail_perm = false;
	int trail_order = 0;
	// encode_from_planes (ckl_recompress.hip's road): there is no volume.  The planes stand in d_planes (planes_stats, count_v /
	// count_h as for cached planes) and the label stage takes every component's label from these run tables of a decode
	// session (ckl_recompress.hpp).  Set for the length of that call only.
	const ckl::dev::RunLabels* label_src = nullptr;
	std::vector<std::pair<const char*, double>> host_marks;      // the host timer's marks of that run: read by ckl_recompress.hip's profile line (CKL_PROFILE), by nothing else
	VolumeStats planes_stats;          // max / pairs of the volume the cached planes were built from
	int64_t planes_dims[3] = { 0, 0, 0 };
	// trail graph (ckl_trail.hpp)
	std::vector<uint32_t> count_special, count_corner;
	DevBuf<uint32_t> d_plane_partial, t_blk_special, t_blk_corner;
	DevBuf<unsigned long long> d_plane_partial_max, d_plane_out;
	uint32_t graph_blocks = 0;
	uint32_t tiles_x = 0, tiles_y = 0, mtx2 = 0;
	uint64_t adjm_stride = 0;
	bool graph_permissible = false;
	bool planes_deferred = false;      // planes_pass left its counts on the device: graph_pass (or planes_collect) fetches them
	bool trail_zeroed = false;         // trail_prezero() ran on the stream since the last trail: crack_pass skips its fills
	DevBuf<uint64_t> t_nbase, t_cobase, t_ibase;
	DevBuf<uint32_t> t_ncap, t_cocap, t_icap, t_max_steps;
	bool emit_fused = false;                     // the last crack pass that built a trail emitted it with k_trail_emit (emit_plan, ckl_encode.hip)
	size_t emit_lds = 0;                         // ... the LDS its plan asked for, static + dynamic
	size_t last_trail_slices = 0;                // slices of the last crack pass (the layout of t_counters)
	DevBuf<uint32_t> t_counters;                 // n_nodes | n_snap | n_corners | n_starts | n_items | n_events | seg_len_sum, [nslices] each
	DevBuf<uint32_t> t_node_vertex, t_vert2node, t_corner_vertex;
	DevBuf<uint8_t> t_node_adj;
	DevBuf<uint32_t> t_dart_end, t_dart_len, t_dart_minv, t_dart_minpos, t_parent, t_start_bits, t_starts;
	DevBuf<uint4> t_dart_codes;
	DevBuf<uint8_t> t_dart_inline;
	DevBuf<unsigned long long> t_compmin;
	DevBuf<uint32_t> t_items, t_item_off, t_chain_item0, t_events, t_chain_ev0, t_ev_lnd, t_ev_item;

	~ckl_encoder() {
		if (ev0) (void)hipEventDestroy(ev0);
		if (ev1) (void)hipEventDestroy(ev1);
		if (evd0) (void)hipEventDestroy(evd0);
		if (evd1) (void)hipEventDestroy(evd1);
		if (ev_in) (void)hipEventDestroy(ev_in);
		if (ev_prezero) (void)hipEventDestroy(ev_prezero);
		// the buffers below go back to a pool that other threads' sessions draw from: nothing of this session may
		// still be queued then (a run that ended in an error leaves its streams as they were)
		if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
		if (stream2) { (void)hipStreamSynchronize(stream2); (void)hipStreamDestroy(stream2); }
		if (stream_copy) { (void)hipStreamSynchronize(stream_copy); (void)hipStreamDestroy(stream_copy); }
		if (stream_tab) { (void)hipStreamSynchronize(stream_tab); (void)hipStreamDestroy(stream_tab); }
		if (ev_codes) (void)hipEventDestroy(ev_codes);
		if (tables_staging) ckl::host_out_free(tables_staging);
		if (ev_labels_crc) (void)hipEventDestroy(ev_labels_crc);
	}
};

namespace ckl {

template <typename T>
inline std::vector<T> download(const T* p, size_t n, hipStream_t s) {
	std::vector<T> h(n);
	if (n) CKL_HIP(hipMemcpyAsync(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost, s));
	CKL_HIP(hipStreamSynchronize(s));
	return h;
}

// wall-clock breakdown of the host side, printed when CKL_PROFILE is set
struct HostTimer {
	bool on;
	std::chrono::steady_clock::time_point t0;
	std::vector<std::pair<const char*, double>> marks;
	HostTimer() : on(getenv("CKL_PROFILE") != nullptr), t0(std::chrono::steady_clock::now()) {}
	void mark(const char* name) {
		if (!on) return;
		auto t1 = std::chrono::steady_clock::now();
		marks.emplace_back(name, std::chrono::duration<double, std::milli>(t1 - t0).count());
		t0 = t1;
	}
	~HostTimer();
};
inline thread_local HostTimer* g_ht = nullptr;      // the running entry point's timer: one for both translation units
#define HT_MARK(name) do { if (g_ht) g_ht->mark(name); } while (0)
inline HostTimer::~HostTimer() {
		g_ht = nullptr;
		if (!on) return;
		fprintf(stderr, "[ckl encode host ms]");
		for (auto& m : marks) fprintf(stderr, " %s=%.2f", m.first, m.second);
		fprintf(stderr, "\n");
}

// a call on a session begins: its device current, its two streams behind the caller's default stream
inline void enter(ckl_encoder* e) {
	if (!e) throw Error(CKL_ERR_ARG, "crackle_amd: null encoder");
	select_device(e->device);
	wait_for_default_stream(e->stream, e->ev_in);
	wait_for_default_stream(e->stream2, e->ev_in);
}

// the previous run's background copy of its codes (ckl_encoder_async_host_copy) is over; `quiet`: on an error path,
// where a second error must not replace the first
inline void drain_host_copy(ckl_encoder& e, bool quiet = false) {
	if (!e.host_copy_pending) return;
	if (quiet) (void)hipStreamSynchronize(e.stream_copy);
	else CKL_HIP(hipStreamSynchronize(e.stream_copy));
	e.host_copy_pending = false;
}

// a copy of the bytes becomes the caller's: *out / *out_len, released with ckl_free
enum class OutAlloc { MALLOC, HOST_OUT };
inline void hand_out(const uint8_t* bytes, size_t n, OutAlloc how, uint8_t** out, uint64_t* out_len) {
	uint8_t* p = static_cast<uint8_t*>(how == OutAlloc::MALLOC ? malloc(n ? n : 1) : host_out_alloc(n ? n : 1));
	if (!p) throw Error(CKL_ERR_RUNTIME, "crackle_amd: out of host memory");
	if (n) memcpy(p, bytes, n);
	*out = p;
	*out_len = n;
}
inline void hand_out(const std::vector<uint8_t>& bin, OutAlloc how, uint8_t** out, uint64_t* out_len) { hand_out(bin.data(), bin.size(), how, out, out_len); }

// the label planes of the session, V then H, as the kernels take them
inline uint32_t* plane_v(const ckl_encoder& e) { return e.d_planes.p; }
inline uint32_t* plane_h(const ckl_encoder& e, uint32_t ns) { return e.d_planes.p + e.plane_words * ns; }

// what every entry point refuses before it asks for a device (ckl_encode.hip)
void check_dims(int64_t sx, int64_t sy, int64_t sz, int dtype_bytes, int is_signed);
// The stream's header as the volume's statistics decide it unless the overrides do; of an empty volume (all statistics 0)
// it is the whole stream.  num_label_bytes comes later.
Header stream_header(int data_width, int64_t sx, int64_t sy, int64_t sz, const VolumeStats& st, bool allow_pins, bool fortran_order, uint64_t markov_model_order, const ckl_encode_overrides* ov);
inline std::vector<uint8_t> header_bytes(const Header& head) {
	std::vector<uint8_t> hb;
	head.write(hb);
	return hb;
}

// Planes that the caller's own kernels write, not planes_pass (ckl_recompress.hip, reencode_markov).  planes_adopt: the
// session takes their geometry and holds room for V | H (plane_v, plane_h) and for d_count_vh, [4][ns], whose first
// count_rows rows are zeroed on the session's stream.  planes_adopt_counts, once the kernels ran: rows 0 and 1 of what
// they left in d_count_vh, fetched by the caller, become the session's count_v and count_h.
void planes_adopt(ckl_encoder& e, uint32_t row_words, uint64_t plane_words, uint32_t ns, uint32_t count_rows);
void planes_adopt_counts(ckl_encoder& e, const std::vector<uint32_t>& counts, uint32_t ns);
// The one door from a decode session's tables into the encoder: the stream of the volume whose planes and counts stand
// adopted in the session, whose statistics are `st` and whose components take their labels from `labels`
// (ckl_recompress.hpp).  FLAT labels, background colour chosen as compress() chooses it.  The session points at `labels`
// for the length of the call only, however it ends.
void encode_from_planes(
	ckl_encoder& e, const dev::RunLabels& labels, int64_t sx, int64_t sy, int64_t sz, int data_width, bool fortran_order,
	uint64_t markov_model_order, const VolumeStats& st, const std::vector<uint32_t>& counts, uint8_t** out, uint64_t* out_len);

// The whole pin stage of a volume that one device holds (ckl_encode_pins.hip, instantiated there for the four label
// widths): the pin label section from the labels, the component id of every voxel and the label of every component
template <typename LABEL>
std::vector<uint8_t> pins_section_plain(
	ckl_encoder& e, const LABEL* labels, const uint32_t* cc, const uint64_t* comp_label, int64_t sx, int64_t sy, int64_t sz, uint64_t N,
	const std::vector<uint32_t>& nc, int index_width, int stored_width, bool auto_bgcolor, int64_t manual_bgcolor);

}  // namespace ckl
