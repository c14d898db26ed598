// The encoder's flat label stage (ckl_encode_labels.hip) as the encoder's schedule (ckl_encode.hip) calls it: the 2-D
// components of every slice with their crcs and labels, enqueued and collected on the session's label stream, the flat
// label section, and the component id of every voxel for those who read the run tables (pins, ckl_encoder_components).
// What the stage keeps between its calls is the session's LabelStage (ckl_encoder.hpp).
#pragma once

#include "ckl_encoder.hpp"

namespace ckl {

// LDS that the label stream's kernels keep to when they run beside two walks per CU (k_strip_ccl_enc, k_slice_resolve_enc):
// label_start (ckl_encode.hip) lets the stream start with the walk only where this fits beside them
constexpr size_t kFlatResolveLds = 40960;

struct FlatResult {
	std::vector<uint32_t> ncomp;      // per slice
	std::vector<uint32_t> crcs;       // per slice crc32c of the component image
	uint64_t total = 0;               // components over all slices; mapping stays in e.d_mapping
};

// The label stage of a volume (labels.hpp:56-88): the 2-D components of every slice, their count, the crc32c of the
// component image and the label of every component.  Enqueued on the label stream; the results are collected
// (flat_collect) while the crack trail runs on the other stream.  Flat labels come from the strip kernels
// (ckl_strips.hpp): k_strip_ccl_enc labels each strip of rows in LDS, k_slice_resolve_enc joins the strips of a slice —
// tables per strip component, not per run.  need_runs: the caller reads the run tables afterwards (pins and
// ckl_encoder_components paint the component volume from run_cc); those and what flat_strip_plan turns down take the
// run pipeline.
// beside_walk: the stage starts with the trail's serial walk, which leaves the chip to it.  Only then do the strips take
// it: in front of the graph kernel (large slices, many nodes) the strip kernel shares the chip with kernels that fill it,
// and the trail paid for it in full when that was tried at C2; those volumes stay as they were.
void flat_enqueue(ckl_encoder& e, const void* labels, int64_t sx, int64_t sy, int64_t sz, bool need_runs, bool beside_walk);
// component counts, crcs, component -> label (labels.hpp:71-88); label_width: bytes of a label of `labels`
void flat_collect(ckl_encoder& e, const void* labels, int label_width, int64_t sx, int64_t sy, int64_t sz, FlatResult& out);
// The flat label section (labels.hpp:92-152) on device: sort + unique of the component
// labels, keys by binary search, everything packed at its byte width into e.d_labels_bin.
// Returns the section size; num_unique comes back for the header arithmetic only.
uint64_t flat_section(ckl_encoder& e, uint64_t N, int stored_width, int component_width, uint32_t ns, const ckl_encode_overrides* ov = nullptr);
// Global component id (+ id_base) of every voxel into cc_device, on the label stream, from the run tables that a stage
// enqueued with need_runs and then collected has left
void paint_components(ckl_encoder& e, int64_t sx, int64_t sy, int64_t sz, uint32_t id_base, uint32_t* cc_device);

}  // namespace ckl
