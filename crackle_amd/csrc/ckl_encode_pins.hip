// The pin stage of the encoder on the device (labels.hpp:157-344, pins.hpp:95-403): the column passes of
// ckl_pins_dev.hpp over a resident label volume and its component ids, for one device (pins_section_plain,
// ckl_encoder_pin_labels) and sharded by rows (ckl_pins_rows_*).  The ordered cover runs on the host (ckl_pins.hip).
#include "ckl_encoder.hpp"
#include "ckl_pins_dev.hpp"

#include <algorithm>
#include <functional>
#include <memory>

using namespace ckl;
using namespace ckl::dev;

namespace {

// the labels with the key of their first column run (the order they enter `pinsets`, src/pins.hpp:126-163), from the
// components' labels and first runs on the device
// The labels with their first column runs (k_pin_label_first / _list) in two steps: the kernels, enqueued as soon as
// first_any is final (behind the first column pass), and the collection of the two short lists — on a stream of its
// own, so that it does not queue behind the passes that follow on the label stream.
struct PinLabelLists {
	DevBuf<uint64_t> d_tab;
	DevBuf<uint32_t> d_count;
	uint32_t slots = 0;
	hipEvent_t ready = nullptr;
	~PinLabelLists() { if (ready) (void)hipEventDestroy(ready); }
};
void pin_label_table_enqueue(ckl_encoder& e, const uint64_t* comp_label, const uint64_t* first_any_dev, uint64_t N, PinLabelLists& t) {
	hipStream_t s = e.stream2;
	if (N > (1ull << 30)) throw Error(CKL_ERR_RUNTIME, "crackle_amd: too many components for pin labels");
	uint32_t slots = 1024;
	while (slots < 2 * N) slots <<= 1;
	t.slots = slots;
	t.d_tab.ensure(4ull * slots + 1);      // keys | values | label list | first list, + the all-ones label's minimum
	t.d_count.ensure(1);
	CKL_HIP(hipMemsetAsync(t.d_tab.p, 0xFF, (2ull * slots) * sizeof(uint64_t), s));
	CKL_HIP(hipMemsetAsync(t.d_tab.p + 4ull * slots, 0xFF, sizeof(uint64_t), s));
	CKL_HIP(hipMemsetAsync(t.d_count.p, 0, sizeof(uint32_t), s));
	unsigned long long* tab = reinterpret_cast<unsigned long long*>(t.d_tab.p);
	hipLaunchKernelGGL(k_pin_label_first, dim3(static_cast<uint32_t>((N + kPinBlock - 1) / kPinBlock)), dim3(kPinBlock), 0, s,
		reinterpret_cast<const unsigned long long*>(comp_label), reinterpret_cast<const unsigned long long*>(first_any_dev), N, tab, tab + slots, slots - 1u, tab + 4ull * slots);
	hipLaunchKernelGGL(k_pin_label_list, dim3((slots + kPinBlock - 1) / kPinBlock), dim3(kPinBlock), 0, s, tab, tab + slots, slots, t.d_count.p, tab + 2ull * slots, tab + 3ull * slots);
	if (!t.ready) CKL_HIP(hipEventCreateWithFlags(&t.ready, hipEventDisableTiming));
	CKL_HIP(hipEventRecord(t.ready, s));
}
void pin_label_table_collect(ckl_encoder& e, PinLabelLists& t, PinCandidates& pc) {
	if (!e.stream_tab) CKL_HIP(hipStreamCreateWithFlags(&e.stream_tab, hipStreamNonBlocking));
	hipStream_t s = e.stream_tab;
	CKL_HIP(hipStreamWaitEvent(s, t.ready, 0));
	const uint32_t nl = download(t.d_count.p, 1, s)[0];
	pc.label_value = download(t.d_tab.p + 2ull * t.slots, nl, s);
	pc.label_first = download(t.d_tab.p + 3ull * t.slots, nl, s);
	const uint64_t max_first = download(t.d_tab.p + 4ull * t.slots, 1, s)[0];
	if (max_first != kPinNoKey) { pc.label_value.push_back(kPinNoKey); pc.label_first.push_back(max_first); }
}
void pin_label_table(ckl_encoder& e, const uint64_t* comp_label, const uint64_t* first_any_dev, uint64_t N, PinCandidates& pc) {
	PinLabelLists t;
	pin_label_table_enqueue(e, comp_label, first_any_dev, N, t);
	pin_label_table_collect(e, t, pc);
}

// extract_columns + add_pin (src/pins.hpp:95-163) over the rows of `v`: the kept runs marked in v.mark
template <typename LABEL>
void pin_dedup_pass(ckl_encoder& e, const LABEL* labels, const PinVolume& v) {
	hipStream_t s = e.stream2;
	const bool by_thread = getenv("CKL_PINS_ROW_THREADS") != nullptr;      // testing: the general kernel on small volumes
	if (v.sz <= 1024u && !by_thread) {
		// a wavefront per row, label tables in registers
		const dim3 wgrid((v.sy + kPinWaves - 1) / kPinWaves), wblock(64 * kPinWaves);
		// four columns per load where the rows allow it
		// (2048 x 2048 x 256 uint32, the kernel alone: 19.9 ms with one column per load, 9.2 with four, 9.3 / 9.6 with 8 / 16)
		const bool groups = v.sx % 4u == 0 && (reinterpret_cast<uintptr_t>(labels) % (4 * sizeof(LABEL))) == 0 && !getenv("CKL_PINS_COLUMN_LOADS");
#define CKL_DEDUP(K) do { \
			if (groups) hipLaunchKernelGGL((k_pin_dedup_wave<LABEL, K, 4>), wgrid, wblock, 0, s, labels, v); \
			else hipLaunchKernelGGL((k_pin_dedup_wave<LABEL, K, 1>), wgrid, wblock, 0, s, labels, v); \
		} while (0)
		if (v.sz <= 64u) CKL_DEDUP(1);
		else if (v.sz <= 128u) CKL_DEDUP(2);
		else if (v.sz <= 256u) CKL_DEDUP(4);
		else if (v.sz <= 512u) CKL_DEDUP(8);
		else CKL_DEDUP(16);
#undef CKL_DEDUP
	}
	else {
		// taller volumes: a thread per row with its label tables in global memory
		uint32_t cap = 16;
		while (cap < 2u * v.sz) cap <<= 1;
		const uint64_t slots = 2ull * cap * v.sy;
		e.d_pin_tables.ensure(slots * sizeof(PinSlot));
		CKL_HIP(hipMemsetAsync(e.d_pin_tables.p, 0, slots * sizeof(PinSlot), s));
		hipLaunchKernelGGL(k_pin_dedup<LABEL>, dim3((v.sy + kPinRowBlock - 1) / kPinRowBlock), dim3(kPinRowBlock), 0, s,
			labels, v, reinterpret_cast<PinSlot*>(e.d_pin_tables.p), cap);
	}

}

// extract_columns / compute_multiverse / the component -> pin choice of find_suboptimal_pins
// (src/pins.hpp:95-198, 300-346) as device passes over the resident label volume and
// the component id volume (ckl_pins_dev.hpp); only per-component facts and the chosen pins are copied out.
template <typename LABEL>
void pin_passes_device(
	ckl_encoder& e, const LABEL* labels, const uint32_t* cc /* device: component id of every voxel */,
	int64_t sx_, int64_t sy_, int64_t sz_, uint64_t N, PinVolume& v, unsigned long long*& choice, const uint64_t*& first_any,
	const std::function<void(const uint64_t*)>& first_any_final = std::function<void(const uint64_t*)>()      // called (with first_any) once the pass that completes it is enqueued
) {
	hipStream_t s = e.stream2;
	v = PinVolume();
	v.sx = static_cast<uint32_t>(sx_); v.sy = static_cast<uint32_t>(sy_); v.sz = static_cast<uint32_t>(sz_);
	v.sxy = static_cast<uint64_t>(v.sx) * v.sy;
	const uint64_t voxels = v.sxy * v.sz;
	if (v.sz > 65535u) throw Error(CKL_ERR_ARG, "crackle_amd: pin labels need at most 65535 slices");      // the kept marks hold depth + 1 in 16 bits
	const uint64_t mark_words = (voxels + 1) / 2;
	e.d_pin_kept.ensure(mark_words);
	CKL_HIP(hipMemsetAsync(e.d_pin_kept.p, 0, mark_words * sizeof(uint32_t), s));
	v.cc = cc; v.mark = reinterpret_cast<uint16_t*>(e.d_pin_kept.p);

	pin_dedup_pass<LABEL>(e, labels, v);

	e.d_pin_u64.ensure(4 * N + 1);
	e.d_pin_u32.ensure(N + 1);
	PinComponentArrays a;
	a.first_any = reinterpret_cast<unsigned long long*>(e.d_pin_u64.p);
	a.first_kept = a.first_any + N;
	a.best = a.first_kept + N;
	choice = a.best + N;
	first_any = reinterpret_cast<const uint64_t*>(a.first_any);
	a.first_depth = e.d_pin_u32.p;
	CKL_HIP(hipMemsetAsync(a.first_any, 0xFF, 2 * N * sizeof(uint64_t), s));
	CKL_HIP(hipMemsetAsync(a.best, 0, N * sizeof(uint64_t), s));
	CKL_HIP(hipMemsetAsync(a.first_depth, 0, N * sizeof(uint32_t), s));
	const dim3 cgrid((v.sx + kPinBlock - 1) / kPinBlock, v.sy);
	hipLaunchKernelGGL((k_pin_columns<LABEL, 0>), cgrid, dim3(kPinBlock), 0, s, labels, v, a);
	if (first_any_final) first_any_final(first_any);
	hipLaunchKernelGGL((k_pin_extent<LABEL, true>), dim3(static_cast<uint32_t>((N + kPinBlock - 1) / kPinBlock)), dim3(kPinBlock), 0, s,
		labels, v, a.first_kept, static_cast<uint32_t>(N), a.first_depth);
	hipLaunchKernelGGL((k_pin_columns<LABEL, 2>), cgrid, dim3(kPinBlock), 0, s, labels, v, a);
	hipLaunchKernelGGL(k_pin_choice, dim3(static_cast<uint32_t>((N + kPinBlock - 1) / kPinBlock)), dim3(kPinBlock), 0, s, a, N, choice);
}

// `v`, `choice`, `first_any`: of the pin_passes_device call that has run already
template <typename LABEL>
PinCandidates pin_candidates_device(
	ckl_encoder& e, const LABEL* labels, const uint64_t* comp_label /* device: label of every component */, uint64_t N,
	const PinVolume& v, unsigned long long* choice, const uint64_t* first_any
) {
	hipStream_t s = e.stream2;
	CKL_HIP(hipStreamSynchronize(s));
	HT_MARK("p:passes");
	PinCandidates pc;
	pc.comp_label = download(comp_label, N, s);
	pc.comp_first = download(first_any, N, s);
	std::vector<uint64_t> chosen = download(reinterpret_cast<const uint64_t*>(choice), N, s);

	HT_MARK("p:d2h");
	if (N >= kPinNone) throw Error(CKL_ERR_RUNTIME, "crackle_amd: too many pins");
	// The pins: by default every component's pin is an entry of its own (the same run may appear several
	// times: a pin is taken at most once, since taking it removes every component that maps to it) and no
	// sorting is needed.  The ids of a run are then stored once per component that chose it — volumes
	// with long z-runs could reach N x sz ids — so when the entries' ids pass a budget the chosen runs
	// are reduced to the distinct ones first (a sort of the keys on the host).
	uint32_t P = static_cast<uint32_t>(N);
	std::vector<uint64_t> pin_key(chosen);      // key of pin p (identity mapping: the component's choice)
	pc.comp_pin.assign(N, kPinNone);
	for (uint32_t c = 0; c < P; c++) if (chosen[c] != kPinNoKey) pc.comp_pin[c] = c;
	{
		DevBuf<uint32_t> d_ze0;
		d_ze0.ensure(P);
		CKL_HIP(hipMemsetAsync(d_ze0.p, 0, static_cast<size_t>(P) * sizeof(uint32_t), s));
		hipLaunchKernelGGL((k_pin_extent<LABEL, false>), dim3((P + kPinBlock - 1) / kPinBlock), dim3(kPinBlock), 0, s, labels, v, choice, P, d_ze0.p);
		pc.pin_ze = download(d_ze0.p, P, s);
	}
	uint64_t id_total = 0;
	for (uint32_t c = 0; c < P; c++) if (chosen[c] != kPinNoKey) id_total += pc.pin_ze[c] - static_cast<uint32_t>(chosen[c] % v.sz) + 1u;
	uint64_t id_budget = 1ull << 26;      // 256 MiB of ids
	if (const char* env = getenv("CKL_PIN_IDS_BUDGET")) id_budget = static_cast<uint64_t>(std::max(0, atoi(env)));      // testing: forces the distinct-pin path
	DevBuf<unsigned long long> d_key2;
	const unsigned long long* key_dev = choice;
	if (id_total > id_budget) {
		std::vector<uint32_t> order;
		order.reserve(P);
		for (uint32_t c = 0; c < P; c++) if (chosen[c] != kPinNoKey) order.push_back(c);
		std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return chosen[a] != chosen[b] ? chosen[a] < chosen[b] : a < b; });
		std::vector<uint64_t> keys2;
		std::vector<uint32_t> ze2;
		for (size_t i = 0; i < order.size(); i++) {
			const uint32_t c = order[i];
			if (i == 0 || chosen[c] != chosen[order[i - 1]]) { keys2.push_back(chosen[c]); ze2.push_back(pc.pin_ze[c]); }
			pc.comp_pin[c] = static_cast<uint32_t>(keys2.size() - 1);
		}
		pin_key.swap(keys2);
		pc.pin_ze.swap(ze2);
		P = static_cast<uint32_t>(pin_key.size());
		d_key2.ensure(std::max<size_t>(P, 1));
		if (P) CKL_HIP(hipMemcpyAsync(d_key2.p, pin_key.data(), static_cast<size_t>(P) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
		key_dev = d_key2.p;
	}
	pc.pin_x.assign(P, 0); pc.pin_y.assign(P, 0); pc.pin_zs.assign(P, 0);
	for (uint32_t p = 0; p < P; p++) {
		if (pin_key[p] == kPinNoKey) continue;
		const uint64_t col = pin_key[p] / v.sz;
		pc.pin_zs[p] = static_cast<uint32_t>(pin_key[p] % v.sz);
		pc.pin_x[p] = static_cast<uint32_t>(col % v.sx);
		pc.pin_y[p] = static_cast<uint32_t>(col / v.sx);
	}
	HT_MARK("p:keys");
	pc.pin_ids_off.assign(static_cast<size_t>(P) + 1, 0);
	{
		DevBuf<uint64_t> d_off;
		DevBuf<uint32_t> d_ze, d_ids;
		for (uint32_t p = 0; p < P; p++) {
			if (pin_key[p] == kPinNoKey) { pc.pin_ze[p] = pc.pin_zs[p]; pc.pin_ids_off[p + 1] = pc.pin_ids_off[p]; }
			else pc.pin_ids_off[p + 1] = pc.pin_ids_off[p] + (pc.pin_ze[p] - pc.pin_zs[p] + 1u);
		}
		upload(d_off, pc.pin_ids_off, s);
		upload(d_ze, pc.pin_ze, s);
		d_ids.ensure(pc.pin_ids_off[P] + 1);
		if (P) hipLaunchKernelGGL(k_pin_ids, dim3((P + kPinBlock - 1) / kPinBlock), dim3(kPinBlock), 0, s, v, key_dev, d_ze.p, d_off.p, P, d_ids.p);
		pc.pin_ids = download(d_ids.p, pc.pin_ids_off[P], s);
	}
	pin_label_table(e, comp_label, first_any, N, pc);
	HT_MARK("p:ids");
	return pc;
}

// ---- the pin stage sharded by ROWS (config C4 on several GPUs) -----------------------------------------------------
// Candidate pins are z-runs per (x, y) column over the WHOLE volume, so a z-slab cannot find them; a slab of rows
// [y0, y0 + rows) of every slice can: extract_columns / add_pin compare a run only with the label's last pin in the
// previous column of the same row (src/pins.hpp:134-160), so rows are independent, and what is kept per COMPONENT
// (a component lies in one slice but spans rows) is an extremum over its voxels:
//   first_any   smallest key of a run starting in the component                          -> minimum over the ranks
//   first_kept  smallest key of a kept run containing it, with that run's depth          -> minimum of key << 16 | depth
//   best        1 + largest key of a kept run deeper than the first kept one (0: none)   -> maximum, once every rank knows
//                                                                                           the first run's depth
//   z_e + 1     last slice of the chosen run, known to the rank that holds its row        -> maximum (0 elsewhere)
//   ids         component ids along the chosen run, likewise                              -> maximum (0 elsewhere)
// The caller (crackle_amd/distributed.py) holds the arrays in its device memory, reduces them over its process group
// between the calls (RCCL all_reduce of N-entry arrays: 13 MB each for C4's 1.6 M components) and hands the reduced
// arrays back; rank 0 finally runs the ordered cover (ckl_pins_rows_section).  Keys name columns of the whole volume.
template <typename LABEL>
PinVolume pin_rows_volume(ckl_encoder& e, const uint32_t* cc, int64_t sx, int64_t rows, int64_t sz, int64_t y0, bool fresh_marks) {
	PinVolume v;
	v.sx = static_cast<uint32_t>(sx); v.sy = static_cast<uint32_t>(rows); v.sz = static_cast<uint32_t>(sz);
	v.sxy = static_cast<uint64_t>(v.sx) * v.sy;
	v.key_col0 = static_cast<uint64_t>(y0) * v.sx;
	if (v.sz > 65535u) throw Error(CKL_ERR_ARG, "crackle_amd: pin labels need at most 65535 slices");
	const uint64_t mark_words = (v.sxy * v.sz + 1) / 2;
	if (fresh_marks) {
		e.d_pin_kept.ensure(mark_words);
		CKL_HIP(hipMemsetAsync(e.d_pin_kept.p, 0, mark_words * sizeof(uint32_t), e.stream2));
	}
	else if (!e.d_pin_kept.p || e.d_pin_kept.n < mark_words) throw Error(CKL_ERR_ARG, "crackle_amd: ckl_pins_rows_first has to run first");
	v.cc = cc; v.mark = reinterpret_cast<uint16_t*>(e.d_pin_kept.p);
	return v;
}

template <typename LABEL>
void pins_rows_first(ckl_encoder& e, const LABEL* labels, const uint32_t* cc, int64_t sx, int64_t rows, int64_t sz, int64_t y0, uint64_t N,
	uint64_t* first_any, uint64_t* first_kept_packed, uint64_t* comp_label) {
	hipStream_t s = e.stream2;
	const PinVolume v = pin_rows_volume<LABEL>(e, cc, sx, rows, sz, y0, true);
	const uint32_t nb = static_cast<uint32_t>((N + kPinBlock - 1) / kPinBlock);
	// the label of every component that shows in these rows (0 elsewhere: the ranks' arrays merge by maximum)
	e.d_slice_err2.ensure(1);
	CKL_HIP(hipMemsetAsync(comp_label, 0, N * sizeof(uint64_t), s));
	CKL_HIP(hipMemsetAsync(e.d_slice_err2.p, 0, sizeof(uint32_t), s));
	const uint64_t voxels = v.sxy * v.sz;
	const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((voxels + kPinBlock - 1) / kPinBlock, 0x7FFFFFFFull));
	hipLaunchKernelGGL(k_pin_component_labels<LABEL>, dim3(blocks), dim3(kPinBlock), 0, s, labels, cc, voxels, v.sx, N, reinterpret_cast<unsigned long long*>(comp_label), e.d_slice_err2.p);
	pin_dedup_pass<LABEL>(e, labels, v);
	e.d_pin_u64.ensure(N + 1);
	e.d_pin_u32.ensure(N + 1);
	PinComponentArrays a;
	a.first_any = reinterpret_cast<unsigned long long*>(first_any);
	a.first_kept = reinterpret_cast<unsigned long long*>(e.d_pin_u64.p);
	a.best = nullptr;
	a.first_depth = e.d_pin_u32.p;
	CKL_HIP(hipMemsetAsync(a.first_any, 0xFF, N * sizeof(uint64_t), s));
	CKL_HIP(hipMemsetAsync(a.first_kept, 0xFF, N * sizeof(uint64_t), s));
	CKL_HIP(hipMemsetAsync(a.first_depth, 0, N * sizeof(uint32_t), s));
	const dim3 cgrid((v.sx + kPinBlock - 1) / kPinBlock, v.sy);
	hipLaunchKernelGGL((k_pin_columns<LABEL, 0>), cgrid, dim3(kPinBlock), 0, s, labels, v, a);
	hipLaunchKernelGGL((k_pin_extent<LABEL, true>), dim3(nb), dim3(kPinBlock), 0, s, labels, v, a.first_kept, static_cast<uint32_t>(N), a.first_depth);
	hipLaunchKernelGGL(k_pin_pack_first, dim3(nb), dim3(kPinBlock), 0, s, a.first_kept, a.first_depth, N, reinterpret_cast<unsigned long long*>(first_kept_packed));
	if (download(e.d_slice_err2.p, 1, s)[0]) throw Error(CKL_ERR_ARG, "crackle_amd: component id out of range");
}

template <typename LABEL>
void pins_rows_best(ckl_encoder& e, const LABEL* labels, const uint32_t* cc, int64_t sx, int64_t rows, int64_t sz, int64_t y0, uint64_t N,
	const uint64_t* first_kept_packed, uint64_t* best) {
	hipStream_t s = e.stream2;
	const PinVolume v = pin_rows_volume<LABEL>(e, cc, sx, rows, sz, y0, false);
	const uint32_t nb = static_cast<uint32_t>((N + kPinBlock - 1) / kPinBlock);
	e.d_pin_u64.ensure(N + 1);
	e.d_pin_u32.ensure(N + 1);
	PinComponentArrays a;
	a.first_any = nullptr;
	a.first_kept = reinterpret_cast<unsigned long long*>(e.d_pin_u64.p);
	a.best = reinterpret_cast<unsigned long long*>(best);
	a.first_depth = e.d_pin_u32.p;
	hipLaunchKernelGGL(k_pin_unpack_first, dim3(nb), dim3(kPinBlock), 0, s, reinterpret_cast<const unsigned long long*>(first_kept_packed), N, a.first_kept, a.first_depth);
	CKL_HIP(hipMemsetAsync(a.best, 0, N * sizeof(uint64_t), s));
	const dim3 cgrid((v.sx + kPinBlock - 1) / kPinBlock, v.sy);
	hipLaunchKernelGGL((k_pin_columns<LABEL, 2>), cgrid, dim3(kPinBlock), 0, s, labels, v, a);
	CKL_HIP(hipStreamSynchronize(s));
}

template <typename LABEL>
void pins_rows_extent(ckl_encoder& e, const LABEL* labels, const uint32_t* cc, int64_t sx, int64_t rows, int64_t sz, int64_t y0, uint64_t N,
	const uint64_t* first_kept_packed, const uint64_t* best, uint64_t* choice, uint32_t* ze_plus1) {
	hipStream_t s = e.stream2;
	const PinVolume v = pin_rows_volume<LABEL>(e, cc, sx, rows, sz, y0, false);
	const uint32_t nb = static_cast<uint32_t>((N + kPinBlock - 1) / kPinBlock);
	e.d_pin_u64.ensure(N + 1);
	e.d_pin_u32.ensure(N + 1);
	PinComponentArrays a;
	a.first_any = nullptr;
	a.first_kept = reinterpret_cast<unsigned long long*>(e.d_pin_u64.p);
	a.best = reinterpret_cast<unsigned long long*>(const_cast<uint64_t*>(best));
	a.first_depth = e.d_pin_u32.p;
	hipLaunchKernelGGL(k_pin_unpack_first, dim3(nb), dim3(kPinBlock), 0, s, reinterpret_cast<const unsigned long long*>(first_kept_packed), N, a.first_kept, a.first_depth);
	hipLaunchKernelGGL(k_pin_choice, dim3(nb), dim3(kPinBlock), 0, s, a, N, reinterpret_cast<unsigned long long*>(choice));
	CKL_HIP(hipMemsetAsync(ze_plus1, 0, N * sizeof(uint32_t), s));
	hipLaunchKernelGGL((k_pin_extent<LABEL, false, true>), dim3(nb), dim3(kPinBlock), 0, s, labels, v, reinterpret_cast<const unsigned long long*>(choice), static_cast<uint32_t>(N), ze_plus1);
	CKL_HIP(hipStreamSynchronize(s));
}

// The pin label section from the per-component arrays in device memory (every chosen pin an entry of its own:
// pin c is component c's choice): the arrays come to the host in ONE pinned block (host_out_alloc: cached between
// calls), the per-pin bookkeeping runs on the worker threads, pins_cover_host reads the block in place.
// choice[c]: key of the chosen run or kPinNoKey; ze_plus1[c]: its last slice + 1; offsets: N + 1 prefix sums of the
// runs' lengths; ids: the component ids along the runs.
std::vector<uint8_t> pins_section_from_device(
	ckl_encoder& e, int64_t sx, int64_t sy, int64_t sz, uint64_t N, const std::vector<uint32_t>& nc,
	const uint64_t* d_comp_label, const uint64_t* d_first_any, const uint64_t* d_choice, const uint32_t* d_ze_plus1, const uint64_t* d_offsets, const uint32_t* d_ids,
	int stored_width, bool auto_bgcolor, int64_t manual_bgcolor, const PinLabelTable* table = nullptr
) {
	hipStream_t s = e.stream2;
	PinCandidates pc;
	if (!table) pin_label_table(e, d_comp_label, d_first_any, N, pc);      // the labels with their first runs: a few downloads of its own
	const uint64_t total = download(d_offsets + N, 1, s)[0];
	auto up64 = [](uint64_t b) { return (b + 63) & ~static_cast<uint64_t>(63); };
	const uint64_t o_label = 0, o_choice = o_label + up64(N * 8), o_off = o_choice + up64(N * 8), o_ze = o_off + up64((N + 1) * 8), o_ids = o_ze + up64(N * 4);
	const uint64_t o_pins = o_ids + up64(std::max<uint64_t>(total, 1) * 4);      // comp_pin, pin_x, pin_y, pin_zs, pin_ze: written by the host, in the same cached block (no page faults, no zero fill)
	const uint64_t bytes = o_pins + 5 * up64(N * 4);
	struct Block { uint8_t* p = nullptr; hipStream_t s = nullptr; ~Block() { if (p) { (void)hipStreamSynchronize(s); host_out_free(p); } } } blk;      // (copies may still be on their way when an error unwinds)
	blk.s = s;
	blk.p = static_cast<uint8_t*>(host_out_alloc(bytes));
	CKL_HIP(hipMemcpyAsync(blk.p + o_label, d_comp_label, N * 8, hipMemcpyDeviceToHost, s));
	CKL_HIP(hipMemcpyAsync(blk.p + o_choice, d_choice, N * 8, hipMemcpyDeviceToHost, s));
	CKL_HIP(hipMemcpyAsync(blk.p + o_off, d_offsets, (N + 1) * 8, hipMemcpyDeviceToHost, s));
	CKL_HIP(hipMemcpyAsync(blk.p + o_ze, d_ze_plus1, N * 4, hipMemcpyDeviceToHost, s));
	if (total) CKL_HIP(hipMemcpyAsync(blk.p + o_ids, d_ids, total * 4, hipMemcpyDeviceToHost, s));
	uint32_t* const h_comp_pin = reinterpret_cast<uint32_t*>(blk.p + o_pins);
	uint32_t* const h_x = reinterpret_cast<uint32_t*>(blk.p + o_pins + up64(N * 4));
	uint32_t* const h_y = reinterpret_cast<uint32_t*>(blk.p + o_pins + 2 * up64(N * 4));
	uint32_t* const h_zs = reinterpret_cast<uint32_t*>(blk.p + o_pins + 3 * up64(N * 4));
	uint32_t* const h_ze = reinterpret_cast<uint32_t*>(blk.p + o_pins + 4 * up64(N * 4));
	pc.view_comp_pin = h_comp_pin; pc.view_pin_x = h_x; pc.view_pin_y = h_y; pc.view_pin_zs = h_zs; pc.view_pin_ze = h_ze;
	pc.view_components = N;
	pc.view_comp_label = reinterpret_cast<const uint64_t*>(blk.p + o_label);
	pc.view_pin_ids_off = reinterpret_cast<const uint64_t*>(blk.p + o_off);
	pc.view_pin_ids = reinterpret_cast<const uint32_t*>(blk.p + o_ids);
	HT_MARK("p:enqueue");
	const uint64_t* chosen = reinterpret_cast<const uint64_t*>(blk.p + o_choice);
	const uint32_t* ze_plus1 = reinterpret_cast<const uint32_t*>(blk.p + o_ze);
	const uint64_t usx = static_cast<uint64_t>(sx), usz = static_cast<uint64_t>(sz);
	// the copies travel while the cover builds its table of the labels; it calls back when it needs the arrays
	auto arrays_ready = [&]() {
	CKL_HIP(hipStreamSynchronize(s));
	host_parallel_for(N, 65536, [&](size_t lo, size_t hi) {
		for (size_t c = lo; c < hi; c++) {
			if (chosen[c] == kPinNoKey) { h_comp_pin[c] = kPinNone; h_x[c] = h_y[c] = h_zs[c] = h_ze[c] = 0; continue; }
			if (ze_plus1[c] == 0) throw Error(CKL_ERR_RUNTIME, "crackle_amd: a chosen pin lies in no rank's rows");
			h_comp_pin[c] = static_cast<uint32_t>(c);
			const uint64_t col = chosen[c] / usz;
			h_zs[c] = static_cast<uint32_t>(chosen[c] % usz);
			h_ze[c] = ze_plus1[c] - 1u;
			h_x[c] = static_cast<uint32_t>(col % usx);
			h_y[c] = static_cast<uint32_t>(col / usx);
		}
	});
	};
	Header h;
	h.sx = static_cast<uint32_t>(sx); h.sy = static_cast<uint32_t>(sy); h.sz = static_cast<uint32_t>(sz);
	return pins_cover_host(pc, sx, sy, sz, nc, N, h.pin_index_width(), stored_width, auto_bgcolor, manual_bgcolor, arrays_ready, table);
}

}  // namespace

namespace ckl {

// The whole pin stage of a volume that one device holds: the passes of pin_candidates_device, then the chosen
// runs' ends, lengths, offsets (a device scan) and ids without a visit to the host, then pins_section_from_device.
// Volumes whose id lists pass the budget (long z-runs chosen by many components) take pin_candidates_device's
// route, which reduces the chosen runs to the distinct ones first.
template <typename LABEL>
std::vector<uint8_t> pins_section_plain(
	ckl_encoder& e, const LABEL* labels, const uint32_t* cc, const uint64_t* comp_label, int64_t sx, int64_t sy, int64_t sz, uint64_t N,
	const std::vector<uint32_t>& nc, int index_width, int stored_width, bool auto_bgcolor, int64_t manual_bgcolor
) {
	hipStream_t s = e.stream2;
	if (N >= kPinNone) throw Error(CKL_ERR_RUNTIME, "crackle_amd: too many pins");
	unsigned long long* choice = nullptr;
	const uint64_t* first_any = nullptr;
	PinVolume v;
	// The labels' first runs are final after the first column pass: their lists are made there and come to the host
	// on a stream of their own, and the host builds the label table (7 ms at C4) while the later passes still run.
	PinLabelLists lists;
	pin_passes_device<LABEL>(e, labels, cc, sx, sy, sz, N, v, choice, first_any,
		[&](const uint64_t* fa) { pin_label_table_enqueue(e, comp_label, fa, N, lists); });
	const uint32_t nb = static_cast<uint32_t>((N + kPinBlock - 1) / kPinBlock);
	const uint32_t pieces = static_cast<uint32_t>((N + kPinScanPiece - 1) / kPinScanPiece);
	DevBuf<uint32_t> d_zep, d_count, d_ze, d_ids;
	DevBuf<unsigned long long> d_piece, d_off;
	d_zep.ensure(N); d_count.ensure(N); d_piece.ensure(static_cast<size_t>(pieces) + 1); d_off.ensure(N + 1);
	CKL_HIP(hipMemsetAsync(d_zep.p, 0, N * sizeof(uint32_t), s));
	hipLaunchKernelGGL((k_pin_extent<LABEL, false, true>), dim3(nb), dim3(kPinBlock), 0, s, labels, v, choice, static_cast<uint32_t>(N), d_zep.p);
	hipLaunchKernelGGL(k_pin_id_counts, dim3(nb), dim3(kPinBlock), 0, s, choice, d_zep.p, v.sz, N, d_count.p);
	hipLaunchKernelGGL(k_pin_scan_pieces, dim3(pieces), dim3(kPinBlock), 0, s, d_count.p, N, d_piece.p);
	hipLaunchKernelGGL(k_pin_scan_tops, dim3(1), dim3(kPinBlock), 0, s, d_piece.p, pieces);
	hipLaunchKernelGGL(k_pin_scan_offsets, dim3(pieces), dim3(kPinBlock), 0, s, d_count.p, N, d_piece.p, pieces, d_off.p);
	std::shared_ptr<const PinLabelTable> table;
	{
		PinCandidates lc;
		pin_label_table_collect(e, lists, lc);
		HT_MARK("p:lists");
		table = pins_label_table_host(lc.label_value, lc.label_first);
		HT_MARK("p:table");
	}
	const uint64_t total = download(d_off.p + N, 1, s)[0];
	HT_MARK("p:passes");
	uint64_t id_budget = 1ull << 26;      // 256 MiB of ids
	if (const char* env = getenv("CKL_PIN_IDS_BUDGET")) id_budget = static_cast<uint64_t>(std::max(0, atoi(env)));      // testing: forces the distinct-pin path
	if (total > id_budget || getenv("CKL_PINS_HOST_BOOKKEEPING")) {
		const PinCandidates pc = pin_candidates_device<LABEL>(e, labels, comp_label, N, v, choice, first_any);
		HT_MARK("pins_device");
		return pins_cover_host(pc, sx, sy, sz, nc, N, index_width, stored_width, auto_bgcolor, manual_bgcolor);
	}
	d_ze.ensure(N); d_ids.ensure(total + 1);
	hipLaunchKernelGGL(k_pin_minus1, dim3(nb), dim3(kPinBlock), 0, s, d_zep.p, N, d_ze.p);
	hipLaunchKernelGGL(k_pin_ids, dim3(nb), dim3(kPinBlock), 0, s, v, choice, d_ze.p, reinterpret_cast<const uint64_t*>(d_off.p), static_cast<uint32_t>(N), d_ids.p);
	std::vector<uint8_t> bin = pins_section_from_device(e, sx, sy, sz, N, nc, comp_label, first_any, reinterpret_cast<const uint64_t*>(choice), d_zep.p,
		reinterpret_cast<const uint64_t*>(d_off.p), d_ids.p, stored_width, auto_bgcolor, manual_bgcolor, table.get());
	HT_MARK("pins_host");
	return bin;
}

#define CKL_PINS_SECTION(T) template std::vector<uint8_t> pins_section_plain<T>(ckl_encoder&, const T*, const uint32_t*, const uint64_t*, int64_t, int64_t, int64_t, uint64_t, \
	const std::vector<uint32_t>&, int, int, bool, int64_t)
CKL_PINS_SECTION(uint8_t); CKL_PINS_SECTION(uint16_t); CKL_PINS_SECTION(uint32_t); CKL_PINS_SECTION(uint64_t);
#undef CKL_PINS_SECTION

}  // namespace ckl

extern "C" {

int ckl_encoder_pin_labels(
	ckl_encoder* e, const void* labels_device, const uint32_t* cc_device,
	int64_t sx, int64_t sy, int64_t sz, const uint32_t* ncomp_host,
	int stored_width, int auto_bgcolor, int64_t manual_bgcolor,
	uint8_t** out, uint64_t* out_len
) {
	return guard([&] {
		if (!e || !labels_device || !cc_device || !ncomp_host || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		if (sx <= 0 || sy <= 0 || sz <= 0) throw Error(CKL_ERR_ARG, "crackle_amd: empty volume");
		if (sx > 0xFFFFFFFFll || sy > 0xFFFFFFFFll || sz > 0xFFFFFFFFll) throw Error(CKL_ERR_ARG, "crackle_amd: dimensions must fit 32 bits");
		if (stored_width != 1 && stored_width != 2 && stored_width != 4 && stored_width != 8) throw Error(CKL_ERR_ARG, "crackle_amd: stored width must be 1, 2, 4 or 8 bytes");
		enter(e);
		std::vector<uint32_t> nc(ncomp_host, ncomp_host + sz);
		uint64_t N = 0;
		for (uint32_t c : nc) N += c;
		if (N == 0 || N > 0xFFFFFFFFull) throw Error(CKL_ERR_ARG, "crackle_amd: component counts out of range");
		Header h;
		h.sx = static_cast<uint32_t>(sx); h.sy = static_cast<uint32_t>(sy); h.sz = static_cast<uint32_t>(sz);
		hipStream_t s = e->stream2;
		const uint64_t voxels = static_cast<uint64_t>(sx) * sy * sz;
		// label of every component, read where the id changes along x (every component has such a voxel)
		e->d_mapping.ensure(N + 1);
		e->d_slice_err2.ensure(1);
		CKL_HIP(hipMemsetAsync(e->d_mapping.p, 0, N * sizeof(uint64_t), s));
		CKL_HIP(hipMemsetAsync(e->d_slice_err2.p, 0, sizeof(uint32_t), s));
		const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((voxels + kPinBlock - 1) / kPinBlock, 0x7FFFFFFFull));
		with_label_type(e->dtype_bytes, [&](auto t) {
			typedef typename decltype(t)::type T;
			hipLaunchKernelGGL(k_pin_component_labels<T>, dim3(blocks), dim3(kPinBlock), 0, s, reinterpret_cast<const T*>(labels_device), cc_device, voxels, static_cast<uint32_t>(sx), N,
				reinterpret_cast<unsigned long long*>(e->d_mapping.p), e->d_slice_err2.p);
			if (download(e->d_slice_err2.p, 1, s)[0]) throw Error(CKL_ERR_ARG, "crackle_amd: component id out of range");
			hand_out(pins_section_plain<T>(*e, reinterpret_cast<const T*>(labels_device), cc_device, e->d_mapping.p, sx, sy, sz, N, nc, h.pin_index_width(), stored_width, auto_bgcolor != 0, manual_bgcolor),
				OutAlloc::HOST_OUT, out, out_len);
		});
	});
}

static void pins_rows_check(const ckl_encoder* e, const void* labels, const uint32_t* cc, int64_t sx, int64_t rows, int64_t sz, int64_t y0, uint64_t N) {
	if (!e || !labels || !cc) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
	if (sx <= 0 || rows <= 0 || sz <= 0 || y0 < 0) throw Error(CKL_ERR_ARG, "crackle_amd: empty row slab");
	if (sx > 0x7FFFFFF0ll || rows > 0x7FFFFFF0ll || y0 > 0x7FFFFFF0ll || sz > 65535) throw Error(CKL_ERR_ARG, "crackle_amd: row slab dimensions out of range");
	if (N == 0 || N >= kPinNone) throw Error(CKL_ERR_ARG, "crackle_amd: component count out of range");
	if (static_cast<unsigned __int128>(y0 + rows) * static_cast<uint64_t>(sx) * static_cast<uint64_t>(sz) >= (static_cast<unsigned __int128>(1) << 47)) throw Error(CKL_ERR_ARG, "crackle_amd: volume too large for the row-sharded pin stage");
}

int ckl_pins_rows_first(ckl_encoder* e, const void* labels_rows, const uint32_t* cc_rows, int64_t sx, int64_t rows, int64_t sz, int64_t y0, uint64_t n_components,
	uint64_t* first_any, uint64_t* first_kept, uint64_t* comp_label) {
	return guard([&] {
		pins_rows_check(e, labels_rows, cc_rows, sx, rows, sz, y0, n_components);
		if (!first_any || !first_kept || !comp_label) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		enter(e);
		with_label_type(e->dtype_bytes, [&](auto t) { pins_rows_first(*e, static_cast<const typename decltype(t)::type*>(labels_rows), cc_rows, sx, rows, sz, y0, n_components, first_any, first_kept, comp_label); });
		CKL_HIP(hipStreamSynchronize(e->stream2));
	});
}

int ckl_pins_rows_best(ckl_encoder* e, const void* labels_rows, const uint32_t* cc_rows, int64_t sx, int64_t rows, int64_t sz, int64_t y0, uint64_t n_components,
	const uint64_t* first_kept, uint64_t* best) {
	return guard([&] {
		pins_rows_check(e, labels_rows, cc_rows, sx, rows, sz, y0, n_components);
		if (!first_kept || !best) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		enter(e);
		with_label_type(e->dtype_bytes, [&](auto t) { pins_rows_best(*e, static_cast<const typename decltype(t)::type*>(labels_rows), cc_rows, sx, rows, sz, y0, n_components, first_kept, best); });
	});
}

int ckl_pins_rows_extent(ckl_encoder* e, const void* labels_rows, const uint32_t* cc_rows, int64_t sx, int64_t rows, int64_t sz, int64_t y0, uint64_t n_components,
	const uint64_t* first_kept, const uint64_t* best, uint64_t* choice, uint32_t* ze_plus1) {
	return guard([&] {
		pins_rows_check(e, labels_rows, cc_rows, sx, rows, sz, y0, n_components);
		if (!first_kept || !best || !choice || !ze_plus1) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		enter(e);
		with_label_type(e->dtype_bytes, [&](auto t) { pins_rows_extent(*e, static_cast<const typename decltype(t)::type*>(labels_rows), cc_rows, sx, rows, sz, y0, n_components, first_kept, best, choice, ze_plus1); });
	});
}

int ckl_pins_rows_ids(ckl_encoder* e, const uint32_t* cc_rows, int64_t sx, int64_t rows, int64_t sz, int64_t y0, uint64_t n_components,
	const uint64_t* choice, const uint32_t* ze_plus1, const uint64_t* offsets, uint32_t* ids) {
	return guard([&] {
		if (!e || !cc_rows || !choice || !ze_plus1 || !offsets || !ids) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		if (sx <= 0 || rows <= 0 || sz <= 0 || y0 < 0 || n_components == 0 || n_components >= kPinNone) throw Error(CKL_ERR_ARG, "crackle_amd: row slab out of range");
		enter(e);
		hipStream_t s = e->stream2;
		PinVolume v;
		v.sx = static_cast<uint32_t>(sx); v.sy = static_cast<uint32_t>(rows); v.sz = static_cast<uint32_t>(sz);
		v.sxy = static_cast<uint64_t>(v.sx) * v.sy; v.key_col0 = static_cast<uint64_t>(y0) * v.sx; v.cc = cc_rows; v.mark = nullptr;
		// k_pin_ids wants the last slice itself: the entries that are 0 ("not mine") are skipped by the row check, so ze_plus1 - 1 of the others
		DevBuf<uint32_t> d_ze;
		d_ze.ensure(n_components);
		const uint32_t nb = static_cast<uint32_t>((n_components + kPinBlock - 1) / kPinBlock);
		hipLaunchKernelGGL(k_pin_minus1, dim3(nb), dim3(kPinBlock), 0, s, ze_plus1, n_components, d_ze.p);
		hipLaunchKernelGGL(k_pin_ids, dim3(nb), dim3(kPinBlock), 0, s, v, reinterpret_cast<const unsigned long long*>(choice), d_ze.p, offsets, static_cast<uint32_t>(n_components), ids);
		CKL_HIP(hipStreamSynchronize(s));
	});
}

int ckl_pins_rows_section(ckl_encoder* e, int64_t sx, int64_t sy, int64_t sz, uint64_t n_components, const uint32_t* ncomp_host,
	const uint64_t* comp_label, const uint64_t* first_any, const uint64_t* choice, const uint32_t* ze_plus1, const uint64_t* offsets, const uint32_t* ids,
	int stored_width, int auto_bgcolor, int64_t manual_bgcolor, uint8_t** out, uint64_t* out_len) {
	return guard([&] {
		if (!e || !ncomp_host || !comp_label || !first_any || !choice || !ze_plus1 || !offsets || !ids || !out || !out_len) throw Error(CKL_ERR_ARG, "crackle_amd: null argument");
		if (sx <= 0 || sy <= 0 || sz <= 0) throw Error(CKL_ERR_ARG, "crackle_amd: empty volume");
		if (stored_width != 1 && stored_width != 2 && stored_width != 4 && stored_width != 8) throw Error(CKL_ERR_ARG, "crackle_amd: stored width must be 1, 2, 4 or 8 bytes");
		const uint64_t N = n_components;
		if (N == 0 || N >= kPinNone) throw Error(CKL_ERR_ARG, "crackle_amd: component count out of range");
		enter(e);
		std::vector<uint32_t> nc(ncomp_host, ncomp_host + sz);
		HostTimer ht;
		g_ht = &ht;
		const std::vector<uint8_t> bin = pins_section_from_device(*e, sx, sy, sz, N, nc, comp_label, first_any, choice, ze_plus1, offsets, ids, stored_width, auto_bgcolor != 0, manual_bgcolor);
		ht.mark("p:cover");
		hand_out(bin, OutAlloc::HOST_OUT, out, out_len);
	});
}

}  // extern "C"
