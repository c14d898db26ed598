/* crackle_amd — MI355X-native crackle encode/decode path: C-ABI drop-in boundary.
 *
 * Every entry point replaces (or is the device-resident form of) a function the
 * reference exposes for this path; the reference interface each one stands in
 * for is cited as /root/reference-relative file:line.
 *
 *   reference pybind module   src/fastcrackle.cpp:84-128  (decompress)
 *                             src/fastcrackle.cpp:163-210 (compress)
 *   reference C++ core        src/crackle.hpp:220-257     (crackle::compress<LABEL>)
 *                             src/crackle.hpp:503-663     (crackle::decompress<LABEL,OUT>)
 *   reference C-ABI precedent wasm/crackle_wasm.cc:22-68  (crackle_compress / crackle_decompress)
 *
 * Conventions: plain pointers and sizes only; no exceptions cross the boundary;
 * every function returns a ckl_status and records a thread-local message
 * retrievable with ckl_last_error().  Label volumes are x-fastest ("Fortran
 * order", src/crackle.hpp:219).  All compute runs on the selected HIP device;
 * there is no CPU fallback — without a usable device the calls fail with
 * CKL_ERR_NO_DEVICE.
 *
 * Threads: any number of host threads may be inside the one-shot calls (every
 * function that takes a stream or a volume and a device) at the same time, on the
 * same or on different devices.  A session object (ckl_decoder, ckl_encoder)
 * belongs to one thread at a time: threads may each hold their own, no two may be
 * inside calls on the same session together; a session may be handed from one
 * thread to another between calls.  ckl_last_error() is the calling thread's
 * own.  ckl_free may be called from any thread.  
 */
#ifndef CRACKLE_AMD_H
#define CRACKLE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ckl_status {
	CKL_OK = 0,
	CKL_ERR_FORMAT = 1,     /* not a crackle stream / corrupt header: crackle.FormatError (crackle/headers.py:78-105) */
	CKL_ERR_RUNTIME = 2,    /* std::runtime_error("crackle: ...") in the reference -> RuntimeError */
	CKL_ERR_ARG = 3,        /* bad argument (TypeError/ValueError in the Python shim) */
	CKL_ERR_NO_DEVICE = 4,  /* no usable HIP device: the product path refuses to run on the CPU */
	CKL_ERR_CRC = 5         /* a stored crc32c did not match (the reference swallows these) */
} ckl_status;

/* where a caller-provided buffer lives */
enum { CKL_MEM_HOST = 0, CKL_MEM_DEVICE = 1 };

/* Thread-local message of the last failing call on this thread. */
const char* ckl_last_error(void);

/* ABI version of this library (bumped on any signature change). */
int ckl_abi_version(void);

/* Number of usable HIP devices (0 when none; never fails). */
int ckl_device_count(void);

/* Parsed stream header — replaces crackle::CrackleHeader (src/header.hpp:35-308)
 * and crackle/headers.py:78-124 for callers that need to size outputs. */
typedef struct ckl_header_info {
	uint32_t format_version;
	uint32_t label_format;       /* 0 FLAT, 2 PINS_VARIABLE_WIDTH */
	uint32_t crack_format;       /* 0 IMPERMISSIBLE, 1 PERMISSIBLE */
	uint32_t is_signed;
	uint32_t data_width;
	uint32_t stored_data_width;
	uint32_t sx, sy, sz;
	uint32_t fortran_order;
	uint32_t markov_model_order;
	uint32_t is_sorted;
	uint64_t num_label_bytes;
	uint64_t header_bytes;
} ckl_header_info;

/* Validates magic/version/crc8 exactly as CrackleHeader::assign_from_buffer
 * (src/header.hpp:98-150).  CKL_ERR_FORMAT on failure. */
int ckl_header_info_from_bytes(const uint8_t* buf, uint64_t n, ckl_header_info* out);

/* ---- one-shot entry points ------------------------------------------------ */

/* Replaces fastcrackle.compress (src/fastcrackle.cpp:163-210) /
 * crackle::compress<LABEL> (src/crackle.hpp:220-257).
 *   labels        x-fastest volume of sx*sy*sz elements, dtype_bytes in {1,2,4,8}
 *   labels_mem    CKL_MEM_HOST or CKL_MEM_DEVICE (pointer valid on `device`)
 *   is_signed     must be 0 (crackle/codec.py:720-721 rejects signed input)
 *   allow_pins .. manual_bgcolor   same meaning as the reference's arguments, with two refusals
 *                 (CKL_ERR_ARG): optimize_pins (allow_pins = 2, find_optimal_pins: out of scope) and
 *                 markov_model_order 14 and 15 — the header's four bits allow them
 *                 (src/header.hpp:126,223), but their 4^N x 4 histogram (4 and 16 GiB of counters) is
 *                 more than this encoder keeps on the device; the decoder takes every order
 *   device        HIP device ordinal
 *   out/out_len   library-owned host buffer holding the .ckl bytes; release with ckl_free (only)
 */
int ckl_compress(
	const void* labels, int labels_mem, int dtype_bytes, int is_signed,
	int64_t sx, int64_t sy, int64_t sz,
	int allow_pins, int fortran_order, uint64_t markov_model_order,
	int optimize_pins, int auto_bgcolor, int64_t manual_bgcolor,
	int device, uint8_t** out, uint64_t* out_len);

void ckl_free(void* p);

/* Replaces fastcrackle.decompress (src/fastcrackle.cpp:84-128) /
 * crackle::decompress<LABEL,OUT> (src/crackle.hpp:503-663).
 *   out            sx*sy*(z_end-z_start) elements of data_width bytes (1 byte each
 *                  when has_label), written x-fastest for fortran_order streams and
 *                  transposed (z fastest) otherwise, as crackle.hpp:617-656 does
 *   out_mem        CKL_MEM_HOST or CKL_MEM_DEVICE
 *   z_start,z_end  slice range; z_end < 0 means sz (clamped like crackle.hpp:527-537)
 */
int ckl_decompress(
	const uint8_t* buf, uint64_t n,
	void* out, uint64_t out_capacity_bytes, int out_mem,
	int64_t z_start, int64_t z_end,
	int has_label, uint64_t label,
	int device);

/* ---- resident sessions (inputs already in HBM; what bench.py times) -------- */

typedef struct ckl_decoder ckl_decoder;

/* Parses the stream on the host (header, z-index + crc32c, label section layout —
 * crackle.hpp:262-336, labels.hpp:424-451), uploads it to HBM and allocates the
 * scratch for slices [z_start, z_end). */
int ckl_decoder_create(
	const uint8_t* buf, uint64_t n, int64_t z_start, int64_t z_end,
	int device, ckl_decoder** out);
/* The same for a stream that is resident in HBM already (the encoder's ckl_encoder_device_stream, or a
 * caller that keeps its streams on the device): `stream_device` is used in place — it stays the
 * caller's and must outlive the session — and nothing is uploaded.  The host reads back what
 * crackle::decompress parses before its slice loop (header, z-index, src/crackle.hpp:262-313; label
 * section head, src/labels.hpp:424-451; markov model; crc tail) in three small copies, never the
 * crack codes.  Ordered after the device's default stream. */
int ckl_decoder_create_device(
	const uint8_t* stream_device, uint64_t n, int64_t z_start, int64_t z_end,
	int device, ckl_decoder** out);
/* Runs the device pipeline into a DEVICE output buffer and waits for it. */
int ckl_decoder_run(ckl_decoder* d, void* out_device, uint64_t out_capacity_bytes, int has_label, uint64_t label);
/* Runs only the crack decoder of the session: the two crack bit planes of every slice of the
 * range (crack_code_to_vcg, src/crackle.hpp:414-425, reduced to the two bits per pixel the
 * component labelling reads), left in HBM and owned by the decoder.  Plane V bit (x,y): crack
 * between pixels (x-1,y)|(x,y); plane H bit (x,y): between (x,y-1)|(x,y); rows of *row_words
 * 32-pixel words, *plane_words words per slice, slices consecutive. */
int ckl_decoder_crack_planes(
	ckl_decoder* d, const uint32_t** plane_v_device, const uint32_t** plane_h_device,
	uint32_t* row_words, uint64_t* plane_words);
/* Integrity check of the decoder's z-range without producing the volume (the per-slice part of
 * crackle.check, crackle/codec.py:900-948, which decodes slice by slice and notes the failures):
 * the pipeline runs up to the component ids; slice_errors[i] receives 0 or a combination of
 * CKL_SLICE_* bits for slice z_start + i. */
#define CKL_SLICE_BAD_CODE 0x7u        /* crack code malformed: index, range or capacity */
#define CKL_SLICE_BAD_COMPONENTS 0x8u  /* component count differs from the label section */
#define CKL_SLICE_BAD_CRC 0x10u        /* crc32c of the component image differs from the stored one */
int ckl_decoder_check(ckl_decoder* d, uint32_t* slice_errors, uint64_t capacity);

/* Replaces crackle::operations::voxel_connectivity_graph (src/operations.hpp:667-826, bound at
 * src/fastcrackle.cpp:538-565): one byte per voxel of the decoder's z-range, x fastest, bit0 +x,
 * bit1 -x, bit2 +y, bit3 -y (from the crack planes), and for connectivity 6 bit4 +z / bit5 -z
 * where neighbouring slices carry the same label (first slice -z and last slice +z always set).
 * ckl_decoder_vcg writes into a DEVICE buffer; ckl_voxel_connectivity_graph is the one-shot
 * form over the whole volume with a HOST buffer of sx*sy*sz bytes, ckl_voxel_connectivity_graph_range
 * the same for slices [z_start, z_end) (z_end < 0: to the end), like the reference's binding. */
int ckl_decoder_vcg(ckl_decoder* d, uint8_t* out_device, uint64_t out_capacity_bytes, int connectivity);
int ckl_voxel_connectivity_graph(const uint8_t* buf, uint64_t n, int connectivity, int device, uint8_t* out_host, uint64_t out_capacity_bytes);
int ckl_voxel_connectivity_graph_range(const uint8_t* buf, uint64_t n, int64_t z_start, int64_t z_end, int connectivity, int device, uint8_t* out_host, uint64_t out_capacity_bytes);

/* Replaces crackle::operations::array_equal (src/operations.hpp:1039-1184, bound at
 * src/fastcrackle.cpp:594-618): *equal = 1 when both streams have the same shape, the same number
 * of components in every slice and label_map1[components1] == label_map1[components2] everywhere
 * — the FIRST stream's component -> label table on both sides, as the reference has it (:1163-1164);
 * crackle/operations.py:976-994 compares the label sets before it calls this. */
int ckl_array_equal(const uint8_t* buf1, uint64_t n1, const uint8_t* buf2, uint64_t n2, int device, int* equal);

/* Replaces crackle::operations::mode_pooling_2x2x1 (src/operations.hpp:1201-1304, bound at
 * src/fastcrackle.cpp:620-639): slices [z_start, z_end) are decoded, pooled 2 x 2 in x and y by the
 * reference's rule (a == b ? a : a == c ? a : b == c ? b : d) and every pooled slice is encoded as
 * a one-slice stream of its own.  *out holds the streams one after the other (release with
 * ckl_free), *lengths their `*count` lengths (release with ckl_free as well). */
int ckl_mode_pooling_2x2x1(
	const uint8_t* buf, uint64_t n, int64_t z_start, int64_t z_end, int device,
	uint8_t** out, uint64_t* out_len, uint64_t** lengths, uint64_t* count);

/* Per-label statistics of the decoder's z-range without materialising the volume:
 * replaces crackle::operations::voxel_counts / centroids / bounding_boxes
 * (src/operations.hpp:321-618, bound by src/fastcrackle.cpp:346-420).  The pipeline runs up
 * to the run labels; a kernel over the runs accumulates, per label of the stream's label
 * table (flat: the unique list; pins: the unique list and the background color), the voxel
 * count, the sums of the x, y and z coordinates (centroid = sums / count) and the inclusive
 * box [xmin ymin zmin xmax ymax zmax] (z in whole-volume coordinates; a label absent from the
 * range keeps the reference's initial box: mins 0xFFFFFFFF, maxes 0).  The reference seeds its
 * box map from the unique list only (:561-567): the background color of a pin stream, when it is
 * not in that list, is default-constructed on first use, so its three minima are 0; when it is
 * also absent from the range it has no entry in the reference's map and is reported here with
 * count 0 and an all-zero box (callers drop rows with count == 0 and boxes[0] == 0).
 * Host outputs, any of which may be NULL: labels[capacity] (values as the decoder paints
 * them, sign-extended to 64 bits, ascending as unsigned), counts[capacity],
 * sums[3*capacity], boxes[6*capacity].  *n_labels receives the table size; CKL_ERR_ARG
 * with *n_labels set when capacity is too small. */
int ckl_decoder_label_stats(
	ckl_decoder* d, uint64_t capacity, uint64_t* labels, uint64_t* counts,
	uint64_t* sums, uint32_t* boxes, uint64_t* n_labels);
/* Contact faces between touching labels in the decoder's z-range without materialising the
 * volume: replaces crackle::operations::contacts (src/operations.hpp:850-1021, bound as
 * fastcrackle.contacts, src/fastcrackle.cpp:567-592).  A face between (x,y) and (x+1,y) or
 * (x,y+1) of one slice counts when the two pixels lie in different components of that slice
 * (:950-961, :995-1008: a stream whose label table was rewritten may have touching components of
 * one label, reported as the pair (a, a)); a face between (x,y,z-1) and (x,y,z) counts for z past
 * the first slice of the range when the two labels differ (:963, :1009-1015); faces with a label
 * 0 are dropped (:940-948).  Labels are the values the decoder paints, sign-extended to 64 bits
 * (decode_label_map<uint64_t>, src/crackle.hpp:456-476).  The range is the session's: callers
 * that follow the reference clamp it by its rule first (:878-888).  Host outputs owned by the
 * library, released with ckl_free: *pairs holds 2 * *n_pairs values (a <= b as unsigned),
 * ascending by (a, b); *faces holds 3 * *n_pairs exact face counts (x, y, z) per pair.  The
 * reference adds one float32 area per face instead; areas are the caller's (nx * wy * wz +
 * ny * wx * wz + nz * wx * wy). */
int ckl_decoder_contacts(ckl_decoder* d, uint64_t** pairs, uint64_t** faces, uint64_t* n_pairs);
/* The contingency table (overlap matrix) of two streams of one shape: for every pair of label values
 * (a, b) for which some voxel has label a in the first stream and b in the second, the exact number of
 * such voxels.  Voxels are matched by their (x, y, z); everything but the shape may differ between the
 * streams (widths, signedness, FLAT or pin labels, format version, crack format, markov order, the
 * fortran_order flag), each is read by its own header.  Labels are the values the decoder paints,
 * sign-extended to 64 bits, as ckl_decoder_contacts and ckl_decoder_label_stats report them.  Label 0 is
 * a label like any other and nothing is dropped: the counts sum to the voxels of the range, the sums over
 * b are the voxel counts of the first stream and the sums over a those of the second.  The pair is
 * ordered (a of the first stream, b of the second), not min / max.  Host outputs owned by the library,
 * released with ckl_free: *pairs holds 2 * *n_pairs values, ascending by (a, b) as unsigned; *counts holds
 * *n_pairs voxel counts.  Nothing is decoded to voxels and nothing is sorted on the device: both sessions
 * run up to their run tables, then one kernel intersects the runs of the two streams row by row.
 * Both sessions must be on one device and agree in sx, sy and the number of slices of their ranges (which
 * may start at different z: slice i of the one is compared with slice i of the other), else CKL_ERR_ARG;
 * null arguments are CKL_ERR_ARG.  A damaged slice of either range is reported as ckl_decompress of that
 * stream reports it.  ckl_decoder_last_timing of `a` reports the device span of the whole operation; both
 * sessions remain usable for any other entry point.  (No counterpart in the reference: it has no such
 * entry.) */
int ckl_decoder_overlaps(ckl_decoder* a, ckl_decoder* b, uint64_t** pairs, uint64_t** counts, uint64_t* n_pairs);
/* The one-shot form of ckl_decoder_overlaps over slices [z_start, z_end) of both streams.  Streams that
 * differ in sx, sy or sz are CKL_ERR_ARG, from the two headers alone (ckl_last_error names both shapes).
 * The range is clamped by the rule of the other consumers (operations::get_szr, src/operations.hpp:54-72):
 * a range without a slice, and sz == 0, are CKL_ERR_RUNTIME "crackle: Invalid range: zs - ze"; a stream
 * with sx * sy == 0 and sz > 0 gives an empty table. */
int ckl_overlaps(const uint8_t* buf1, uint64_t n1, const uint8_t* buf2, uint64_t n2,
                 int64_t z_start, int64_t z_end, int device,
                 uint64_t** pairs, uint64_t** counts, uint64_t* n_pairs);
/* Random access to an x, y, z box: replaces CrackleArray.__getitem__ (crackle/array.py:257-285), which
 * decodes the whole slices of the z-range and lets numpy crop them.  The pipeline runs up to the run
 * tables and the component -> label map over the session's z-range (so a damaged slice of the range is
 * reported exactly as by a decode, wherever the box lies), then one kernel paints the pixels
 * [x0, x1) x [y0, y1) of every slice and nothing else.  The output is dense, laid out as ckl_decompress
 * lays out a volume that was the box: wx = x1 - x0, wy = y1 - y0, wz slices; fortran_order streams
 * out[((z - z0) * wy + (y - y0)) * wx + (x - x0)], others out[((x - x0) * wy + (y - y0)) * wz + (z - z0)];
 * data_width bytes per voxel, or one byte (1 where the label is `label`) with has_label.
 * Bounds: 0 <= x0 <= x1 <= sx and likewise y (and z for ckl_cutout), else CKL_ERR_ARG with the axis in
 * ckl_last_error; nothing is clamped (check_bounds, crackle/array.py:529-532).  A capacity below
 * wx * wy * wz * width is CKL_ERR_ARG; an empty box writes nothing and is CKL_OK.
 * ckl_decoder_cutout writes into a DEVICE buffer and reports the kernel as the last stage of
 * ckl_decoder_stage_timing.  (No counterpart in the reference's C++: its binding has no such entry.) */
int ckl_decoder_cutout(ckl_decoder* d, int64_t x0, int64_t x1, int64_t y0, int64_t y1,
                       void* out_device, uint64_t out_capacity_bytes, int has_label, uint64_t label);
/* The one-shot form of ckl_decoder_cutout (crackle/array.py:257-285) over slices [z0, z1): for
 * CKL_MEM_HOST the box alone is allocated on the device and copied to `out`, not the slices it was cut
 * from.  A box that spans the whole plane (x0 = 0, x1 = sx, y0 = 0, y1 = sy) is ckl_decompress of the
 * z-range. */
int ckl_cutout(const uint8_t* buf, uint64_t n, void* out, uint64_t out_capacity_bytes, int out_mem,
               int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1,
               int has_label, uint64_t label, int device);
/* The inverse of ckl_cutout: replaces CrackleArray.__setitem__ (crackle/array.py:287-340, which decodes the
 * slices of the z-range to the host, assigns with numpy, compresses the slab and splices it in with zsplit /
 * zstack).  *out decodes to the volume of `buf` with the box [x0, x1) x [y0, y1) x [z0, z1) overwritten.
 *   box       dense, data_width bytes per voxel, laid out exactly as ckl_cutout lays out its output for the
 *             same stream and box (fortran_order streams x fastest, others z fastest): ckl_paste of
 *             ckl_cutout's output is the identity on the decoded volume
 *   box_mem   CKL_MEM_HOST or CKL_MEM_DEVICE
 *   has_box   0: every voxel of the box becomes `value` and nothing is uploaded (CKL_ERR_ARG when `value` is
 *             beyond the stream's data width)
 * Bounds as for ckl_cutout (CKL_ERR_ARG, nothing is clamped); signed streams are CKL_ERR_ARG (the encoder
 * takes no signed input); an empty box returns a copy of the stream and needs no device.
 * The slices of the z-range are decoded into a slab in HBM (x fastest), one kernel writes the box into it and
 * an encode session reads it there: only the stream and the box cross the link.
 *   version 1, FLAT labels, [z0, z1) not the whole depth: the result is ckl_zstack of ckl_zsplit's
 *     [0, z0), the slab's stream and ckl_zsplit's [z1, sz).  The slab is encoded under the input's crack
 *     format, FLAT labels, markov order and markov model, so z-index entries, crack codes and slice crcs of
 *     the untouched slices are the input's bytes (a damaged slice there is copied unseen; one inside the
 *     range fails as in ckl_decompress); unique list, key widths and stored width are ckl_zstack's.
 *   otherwise (whole depth, pin labels, version 0): the stream ckl_compress gives for the edited volume
 *     under the input's markov order and fortran_order flag: FLAT, version 1, a model of its own.
 * *out is released with ckl_free. */
int ckl_paste(const uint8_t* buf, uint64_t n,
              const void* box, int box_mem, int has_box, uint64_t value,
              int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1,
              int device, uint8_t** out, uint64_t* out_len);
/* Elapsed device time of the last run, from HIP events recorded on the library's
 * own stream around (a) the whole pipeline and (b) the dominant kernel. */
int ckl_decoder_last_timing(const ckl_decoder* d, float* pipeline_ms, float* dominant_kernel_ms);
/* Name and elapsed milliseconds of stage `index` (0-based, in launch order) of the last
 * run; CKL_ERR_ARG past the last stage.  `*name` points to a static string. */
int ckl_decoder_stage_timing(const ckl_decoder* d, int index, const char** name, float* ms);
/* on = 0: the following runs record HIP events only around the whole pipeline (ckl_decoder_last_timing's
 * pipeline_ms stays valid, the per-stage table is empty); on = 1 (the default): also between the kernels.
 * The events between the kernels cost a few microseconds of device time per run.  (No reference counterpart:
 * the reference has no device.) */
int ckl_decoder_set_stage_events(ckl_decoder* d, int on);
void ckl_decoder_destroy(ckl_decoder* d);

typedef struct ckl_encoder ckl_encoder;

/* Allocates device scratch for volumes up to sx*sy*sz of dtype_bytes. */
int ckl_encoder_create(int64_t sx, int64_t sy, int64_t sz, int dtype_bytes, int device, ckl_encoder** out);

/* Optional overrides used when z-slabs of one volume are encoded on several GPUs and
 * merged afterwards: the format decisions that the reference
 * takes from whole-volume reductions (crackle.hpp:48-64, 233-235) are imposed. */
typedef struct ckl_encode_overrides {
	int32_t force_crack_format;      /* -1: decide from this volume; else 0/1 */
	int32_t force_label_format;      /* -1: decide; else 0 (FLAT) / 2 (PINS) */
	int32_t force_stored_width;      /* 0: decide; else 1/2/4/8 */
	int32_t has_model;               /* 1: use `model` (4^order rows x 4 symbol->rank bytes) instead of this volume's statistics */
	const uint8_t* model;
	/* Optional: called once per run, while the crack trail is still executing, with the slab's
	 * distinct labels (host memory; in no particular order when they come straight from the hash
	 * pass: the caller sorts the union anyway).  It returns the sorted unique labels of ALL slabs
	 * (a superset; host memory that stays valid until the run returns); the flat label section
	 * is then written against that list, so that the slabs' sections concatenate without
	 * re-keying.  Return non-zero to abort the run; a list that lacks one of the slab's labels
	 * fails the run with CKL_ERR_ARG.  NULL: the slab's own list is used. */
	int (*merge_unique)(void* ctx, const uint64_t* local_distinct, uint64_t n_local,
	                    const uint64_t** merged_sorted, uint64_t* n_merged);
	void* merge_ctx;
} ckl_encode_overrides;

/* Encodes a DEVICE-resident volume; result is a library-owned (pinned, cached) host buffer: release with ckl_free. */
int ckl_encoder_run(
	ckl_encoder* e, const void* labels_device,
	int64_t sx, int64_t sy, int64_t sz,
	int allow_pins, int fortran_order, uint64_t markov_model_order,
	int optimize_pins, int auto_bgcolor, int64_t manual_bgcolor,
	const ckl_encode_overrides* overrides,
	uint8_t** out, uint64_t* out_len);

/* Sharded encoders place every slab's crack codes at an offset of a shared buffer that is only
 * known once all slabs are encoded.  With defer != 0 the following runs leave the crack codes in
 * HBM (the code region of the returned stream is then unspecified; everything else is as usual)
 * and ckl_encoder_codes_to_host copies them, contiguous in slice order, to where they belong:
 * one transfer over the GPU's own link instead of a transfer and a host copy. */
int ckl_encoder_defer_codes(ckl_encoder* e, int defer);
/* With keep != 0 every following run also leaves the whole stream, byte for byte what it returns on
 * the host, in HBM: the encode -> decode round trip of a device-resident volume then never re-uploads
 * its own bytes.  ckl_encoder_device_stream hands out pointer and length of the last run's stream; the
 * buffer is the session's and valid until its next run or its destruction. */
int ckl_encoder_keep_device_stream(ckl_encoder* e, int keep);
/* With on != 0 (and ckl_encoder_keep_device_stream), ckl_encoder_run returns as soon as the stream is complete
 * in HBM: header, z-index and the slices' crcs are in the returned host buffer, its crack codes (the bulk) and —
 * for flat labels — the label section with its crc32c (taken on the device) are still crossing PCIe on a stream
 * of their own.  ckl_encoder_host_wait blocks until they have arrived; the
 * host bytes must not be read, and the buffer not be freed, before.  In between the caller may decode from
 * ckl_encoder_device_stream or do anything else on the device; the encoder's next run waits by itself.
 * With ckl_encoder_defer_codes the same holds for ckl_encoder_codes_to_host: it starts the copy and returns.
 * (The reference returns host bytes from a synchronous call, src/crackle.hpp:220-257: that is the default.) */
int ckl_encoder_async_host_copy(ckl_encoder* e, int on);
int ckl_encoder_host_wait(ckl_encoder* e);
int ckl_encoder_device_stream(const ckl_encoder* e, const uint8_t** stream_device, uint64_t* n_bytes);
int ckl_encoder_codes_to_host(ckl_encoder* e, uint8_t* dst_host, uint64_t capacity, uint64_t* n_bytes);
/* Page-locks / releases a host range for device transfers (e.g. a shared mapping). */
int ckl_host_register(void* p, uint64_t bytes);
int ckl_host_unregister(void* p);

/* Whole-volume reductions of the encode path, exposed so that sharded encoders can
 * all-reduce them (lib.hpp:224-256): max label, count of equal linear neighbours
 * inside this slab, and the slab's first and last voxel (for the pair that straddles
 * a slab boundary).  labels_device is a DEVICE pointer. */
int ckl_encoder_stats(
	ckl_encoder* e, const void* labels_device, int64_t sx, int64_t sy, int64_t sz,
	uint64_t* max_label, uint64_t* pixel_pairs, uint64_t* first_voxel, uint64_t* last_voxel);

/* Order-N context histogram of this slab's difference-coded crack moves
 * (markov.hpp:193-220): hist must hold 4^order * 4 uint32.  Must follow a
 * ckl_encoder_run-compatible crack pass; see ckl_encoder_run docs in DESIGN.md. */
int ckl_encoder_markov_stats(
	ckl_encoder* e, const void* labels_device, int64_t sx, int64_t sy, int64_t sz,
	int crack_format, uint64_t markov_model_order, uint32_t* hist);

/* Per-voxel component ids of a DEVICE-resident slab, numbered continuously over its slices
 * from id_base (cc3d::connected_components, src/cc3d.hpp:371-400: 4-connected per slice, ids
 * in first-raster-pixel order), copied to host memory (cc_host: sx*sy*sz uint32, x fastest;
 * ncomp_host: sz counts).  The sharded pin encoder (pins::compute, src/pins.hpp:348-403,
 * needs the whole volume's ids on the host that runs the cover solver) calls it per slab. */
int ckl_encoder_components(
	ckl_encoder* e, const void* labels_device, int64_t sx, int64_t sy, int64_t sz,
	uint32_t id_base, uint32_t* cc_host, uint32_t* ncomp_host);

/* As ckl_encoder_components, the ids staying on the device (cc_device: sx*sy*sz uint32). */
int ckl_encoder_components_device(
	ckl_encoder* e, const void* labels_device, int64_t sx, int64_t sy, int64_t sz,
	uint32_t id_base, uint32_t* cc_device, uint32_t* ncomp_host);

/* The pin label section (pins::compute, src/pins.hpp:348-403 + labels::encode_condensed_pins,
 * src/labels.hpp:157-344) of a WHOLE volume whose labels (the session's dtype) and global
 * component ids are resident on the session's device; ncomp_host holds the component count of
 * each of the sz slices.  What ckl_encoder_run does for allow_pins after labelling components,
 * as a stage of its own for the sharded encoder: rank 0 collects the slabs' labels and ids
 * (ckl_encoder_components_device) in its HBM and calls this once.  Column runs, their dedup and
 * the component -> pin choice run on the device, the ordered cover on the host.  *out is
 * released with ckl_free. */
int ckl_encoder_pin_labels(
	ckl_encoder* e, const void* labels_device, const uint32_t* cc_device,
	int64_t sx, int64_t sy, int64_t sz, const uint32_t* ncomp_host,
	int stored_width, int auto_bgcolor, int64_t manual_bgcolor,
	uint8_t** out, uint64_t* out_len);

/* ---- the pin stage sharded by rows (BASELINE.json configs[4] on several GPUs) ----------------------------------
 * pins::compute (src/pins.hpp:348-403) needs every (x, y) column over ALL slices (extract_columns, :95-163), so a
 * z-slab cannot run it; a slab of ROWS can, because add_pin compares a run only with the label's last pin in the
 * previous column of the same row (:134-160).  The sharded encoder transposes its z-slabs of labels and component ids
 * into row slabs (all-to-all over xGMI) and every rank calls these on rows [y0, y0 + rows) of every slice (x fastest,
 * then its rows, then z).  All arrays are DEVICE memory of n_components entries owned by the caller, who reduces them
 * over its ranks between the calls: unsigned minimum for first_any / first_kept, unsigned maximum for comp_label,
 * best, ze_plus1 and ids.  Keys name columns of the whole volume: (y * sx + x) * sz + z_start.
 *   first   -> first_any (smallest key of a run starting in the component), first_kept (smallest key of a kept run
 *              containing it, << 16 | its depth; all ones: none), comp_label (label of the components seen, else 0)
 *   best    first_kept reduced -> best (1 + largest key of a kept run deeper than the first; 0: none)
 *   extent  first_kept, best reduced -> choice (the run find_suboptimal_pins draws per component, :325-340; the same
 *           on every rank) and ze_plus1 (its last slice + 1 where this rank holds its row, else 0)
 *   ids     choice, ze_plus1 reduced, offsets (exclusive prefix of the runs' lengths, n_components + 1 entries) ->
 *           ids (component ids along the runs of this rank's rows; the caller zeroes the array first)
 *   section (one rank) the reduced arrays -> the pin label section (encode_condensed_pins, src/labels.hpp:192-344),
 *           released with ckl_free.  ncomp_host: component count of every slice. */
int ckl_pins_rows_first(ckl_encoder* e, const void* labels_rows, const uint32_t* cc_rows, int64_t sx, int64_t rows, int64_t sz, int64_t y0,
	uint64_t n_components, uint64_t* first_any, uint64_t* first_kept, uint64_t* comp_label);
int ckl_pins_rows_best(ckl_encoder* e, const void* labels_rows, const uint32_t* cc_rows, int64_t sx, int64_t rows, int64_t sz, int64_t y0,
	uint64_t n_components, const uint64_t* first_kept, uint64_t* best);
int ckl_pins_rows_extent(ckl_encoder* e, const void* labels_rows, const uint32_t* cc_rows, int64_t sx, int64_t rows, int64_t sz, int64_t y0,
	uint64_t n_components, const uint64_t* first_kept, const uint64_t* best, uint64_t* choice, uint32_t* ze_plus1);
int ckl_pins_rows_ids(ckl_encoder* e, const uint32_t* cc_rows, int64_t sx, int64_t rows, int64_t sz, int64_t y0,
	uint64_t n_components, const uint64_t* choice, const uint32_t* ze_plus1, const uint64_t* offsets, uint32_t* ids);
int ckl_pins_rows_section(ckl_encoder* e, int64_t sx, int64_t sy, int64_t sz, uint64_t n_components, const uint32_t* ncomp_host,
	const uint64_t* comp_label, const uint64_t* first_any, const uint64_t* choice, const uint32_t* ze_plus1, const uint64_t* offsets, const uint32_t* ids,
	int stored_width, int auto_bgcolor, int64_t manual_bgcolor, uint8_t** out, uint64_t* out_len);

int ckl_encoder_last_timing(const ckl_encoder* e, float* pipeline_ms, float* dominant_kernel_ms);
/* Which walk the last run's crack trail took (create_crack_codes, src/crackcodes.hpp:374-453): slices walked by
 * the hand-scheduled k_trail_walk loop / by the compiled one (slices with too many nodes or events for its
 * 16-bit fields, or a branch stack beyond its LDS part).  Tests assert the path with it; no reference
 * counterpart. */
int ckl_encoder_walk_paths(ckl_encoder* e, uint32_t* fast_slices, uint32_t* compiled_slices);
/* Which kernels packed the last run's crack codes behind the trail's items: *fused = 1 for k_trail_emit (one workgroup
 * per slice, the code points packed in LDS), 0 for k_trail_offsets + k_trail_expand + k_finish (a volume whose largest
 * slice asks for more LDS than two workgroups per CU leave, or CKL_TRAIL_EMIT=0).  *lds_bytes: what k_trail_emit
 * asked for, static + dynamic, on either path.  Tests assert the path with it; no reference counterpart. */
int ckl_encoder_emit_path(const ckl_encoder* e, int* fused, uint64_t* lds_bytes);
/* Diagnostic: the serial crack trail of the last ckl_encoder_run, by kind of step.  counts[5 * z + k] for slice z:
 * k = 0 steps along the only remaining edge of a node, 1 steps that push a branch and pick the lowest edge
 * (create_crack_codes' one real decision, src/crackcodes.hpp:399-433), 2 dead ends (returns to the branch
 * stack), 3 chain ends, 4 the longest run of steps that take no decision.  max_slices: capacity of counts / 5. */
int ckl_encoder_walk_step_kinds(ckl_encoder* e, uint32_t* counts, uint32_t max_slices, uint32_t* n_slices);
void ckl_encoder_destroy(ckl_encoder* e);

/* ---- host-side stream surgery used by the sharded encoder ------------------ */

/* Concatenates FLAT-label streams of consecutive z-slabs (same sx, sy, dtype, crack
 * format, stored width, markov order+model) into the stream the reference would have
 * produced for the whole volume — native form of crackle.operations.zstack
 * (crackle/operations.py:424-548), host only, no device needed. */
int ckl_zstack(
	const uint8_t* const* bufs, const uint64_t* lens, uint64_t count,
	uint8_t** out, uint64_t* out_len);

/* Host stage of the pin label encoder: candidate pins, greedy cover and the condensed
 * pin section — pins::compute with the fast solver (src/pins.hpp:95-198, 300-403) +
 * labels::encode_condensed_pins (src/labels.hpp:157-344).  `labels` (dtype_bytes wide)
 * and `cc` (global component id of every voxel, as crackle::cc3d::connected_components
 * numbers them, src/cc3d.hpp:371-400) are HOST pointers in Fortran order; `ncomp` holds
 * the component count of each of the sz slices.  ckl_encoder_run and ckl_encoder_pin_labels
 * find the candidate pins on the device and share the ordered cover with this function, which
 * finds them with the reference's own loops; it is exported so that the order-sensitive host
 * logic can be tested without a GPU.  *out is released with ckl_free. */
int ckl_pin_labels_host(
	const void* labels, int dtype_bytes, const uint32_t* cc,
	int64_t sx, int64_t sy, int64_t sz, const uint32_t* ncomp,
	int stored_width, int auto_bgcolor, int64_t manual_bgcolor,
	uint8_t** out, uint64_t* out_len);

/* Replaces crackle::operations::point_cloud (src/operations.hpp:183-262, bound as
 * fastcrackle.point_cloud, src/fastcrackle.cpp:315-345) with dual_graph::extract_contours
 * (src/dual_graph.hpp:133-275): the boundary contours of every 2D component of slices
 * [z_start, z_end) (clamped like operations::get_szr; an empty range is an error), as (x, y, z)
 * uint16 triples per label.  `labels` (when has_labels) restricts the output to those labels,
 * skip_background drops label 0.  The labels that own points come back ascending (the reference
 * returns an unordered_map), offsets_out[i] .. offsets_out[i+1] are label i's points in
 * points_out (3 uint16 each), in the order the reference appends them with parallel = 1: slices
 * ascending, components in index order, each component's contours merged as the reference merges
 * them.  The crack codes are decoded and the contours traced on the device (one wavefront per
 * slice).  Release the three arrays with ckl_free. */
int ckl_point_cloud(
	const uint8_t* buf, uint64_t n, int64_t z_start, int64_t z_end,
	const uint64_t* labels, uint64_t n_labels, int has_labels, int skip_background, int device,
	uint64_t** labels_out, uint64_t** offsets_out, uint16_t** points_out, uint64_t* n_out);

/* Replaces crackle::reencode_with_markov_order (src/crackle.hpp:858-984, bound as
 * fastcrackle.reencode_markov, src/fastcrackle.cpp:212-230): the stream with its crack codes
 * stored under another markov model order.  The crack decoder rasterises the codes on the device
 * and the encoder's crack trail writes them out again; label section and crcs are copied.
 * Streams written by the reference encoder or by this library come out byte for byte as the
 * reference's reencode gives them.  *out (pinned host memory) is released with ckl_free. */
int ckl_reencode_markov(const uint8_t* buf, uint64_t n, int markov_model_order, int device, uint8_t** out, uint64_t* out_len);

/* Replaces crackle.operations.recompress (crackle/operations.py:664-857, which decodes slabs to voxels and
 * compresses them again): the stream that ckl_compress gives for the volume `buf` decodes to, with FLAT
 * labels (format version 1) under markov_model_order (< 0: keep the input's), the input's data width and
 * fortran_order flag.  A stream whose label table was rewritten (remap, mask) keeps a crack between every
 * two components that now share a label; this removes them.  No voxel is decoded: the decoder runs up to
 * its run tables and component -> label map (FLAT, pin and version 0 streams), k_label_planes_from_runs
 * writes the encoder's "labels differ" planes, their counts, the pixel pairs and the maximum label from
 * those, and the encoder's own crack and label stages follow, the label stage reading every new component's
 * label at its first pixel through the same tables.  A damaged slice fails as in ckl_decompress; signed
 * streams are CKL_ERR_ARG.  *out is released with ckl_free. */
int ckl_recompress(const uint8_t* buf, uint64_t n, int markov_model_order, int device, uint8_t** out, uint64_t* out_len);

/* Morphological erosion of a stream's labels by one voxel (fastmorph's erode; the reference has no such
 * function): the stream that ckl_compress gives for the eroded volume, written as ckl_recompress writes its own
 * (FLAT labels, format version 1, markov_model_order < 0: keep the input's, the input's data width and
 * fortran_order flag, the stored width of the largest surviving label).  A voxel keeps its label L != 0 iff
 * every neighbour of the structuring element carries L, and becomes 0 otherwise; the element is the 6, 18 or 26
 * (`connectivity`) offsets of {-1, 0, 1}^3 with 0 < |dx| + |dy| + |dz| <= 1, 2, 3.  Labels are compared, not
 * runs or components: cracks between components that share a label erode nothing.  A neighbour outside the
 * volume counts as different, so every voxel on a face of the volume goes; with CKL_ERODE_KEEP_BORDER (the only
 * flag) such neighbours are ignored.  No voxel is decoded: the decoder runs up to its run tables, the keep bit K
 * of every pixel is worked out from the runs (k_erode_run_labels, k_erode_terms, k_erode_keep), the encoder's
 * planes are K ^ K(x - 1) and K ^ K(y - 1) (k_erode_planes), and the encoder's crack and label stages follow,
 * the label stage reading K beside the tables.  FLAT, pin and version 0 streams; signed streams, another
 * connectivity and unknown flags are CKL_ERR_ARG; the stream of an empty volume comes back as ckl_recompress
 * returns it, without a device.  A damaged slice fails as in ckl_decompress.  *out is released with ckl_free. */
#define CKL_ERODE_KEEP_BORDER 1
int ckl_erode(const uint8_t* buf, uint64_t n, int connectivity, int flags, int markov_model_order, int device,
              uint8_t** out, uint64_t* out_len);

/* Morphological dilation of a stream's labels by one voxel (meant as fastmorph's multilabel dilate with
 * background_only; the reference has no such function): the stream that ckl_compress gives for the dilated
 * volume, written as ckl_erode writes its own (FLAT labels, format version 1, markov_model_order < 0: keep the
 * input's, the input's data width and fortran_order flag).  This project's definition, one iteration per call: a
 * voxel whose label is not 0 keeps it.  For a voxel with label 0 the counted neighbours are the 6, 18 or 26
 * (`connectivity`) offsets of ckl_erode's structuring element that lie inside the volume and carry a label other
 * than 0; without any the voxel stays 0, otherwise it takes the label that occurs most often among them, and among
 * labels tied for most often the smallest, compared as unsigned 64-bit values (the tie rule is this project's and
 * was not checked against fastmorph).  Neighbours outside the volume do not exist, so there is no border flag:
 * `flags` must be 0.  Labels are compared, not runs or components.  No voxel is decoded: the decoder runs up to its
 * run tables, the gained pixels are found from "label != 0" bit planes (k_dilate_nonzero, k_dilate_gain), every
 * gained pixel's label is the mode of its neighbours' labels read through the runs (k_dilate_mode), the encoder's
 * planes are written from both (k_dilate_planes), and the encoder's crack and label stages follow, the label stage
 * reading the gained labels beside the tables.  A stream in which nothing is gained comes back as ckl_recompress
 * returns it.  FLAT, pin and version 0 streams; signed streams, another connectivity and flags other than 0 are
 * CKL_ERR_ARG; the stream of an empty volume comes back as ckl_recompress returns it, without a device.  A damaged
 * slice fails as in ckl_decompress.  *out is released with ckl_free. */
int ckl_dilate(const uint8_t* buf, uint64_t n, int connectivity, int flags, int markov_model_order, int device,
               uint8_t** out, uint64_t* out_len);

/* One level of a resolution pyramid (the reference has only mode_pooling_2x2x1's consumer): the stream that
 * ckl_compress gives for the pooled volume, written as ckl_erode writes its own (FLAT labels, format version 1,
 * markov_model_order < 0: keep the input's, the input's data width and fortran_order flag; the crack format is the
 * one the pooled volume itself selects).  (fx, fy, fz) is (2, 2, 1) or (2, 2, 2); the output's shape is ceil(s / f)
 * per axis, an axis of size 0 or 1 keeps its size.  Label 0 is an ordinary label.
 *   (2, 2, 1)  the reference's rule (src/operations.hpp:1254-1293): with a, b, c, d at (x, y), (x + 1, y), (x, y + 1),
 *              (x + 1, y + 1): a == b -> a, a == c -> a, b == c -> b, else d; where the block is cut by an odd sx or
 *              sy, the voxel at its origin is copied.
 *   (2, 2, 2)  the label that occurs most often among the block's voxels that exist (8, or 4, 2, 1 at odd ends); ties
 *              go to the smallest label, compared as unsigned 64-bit values (ckl_dilate's tie rule).  At an odd sz the
 *              last output slice pools 2 x 2 x 1 blocks by this rule, not by the reference's.
 * No voxel is decoded and no dense label volume exists, neither the input's nor the pooled one: the decoder runs up to
 * its run tables, the output words are cut where an input row under them has a break (k_pool_cuts), the rule is
 * evaluated once per cut with one run cursor per input row (k_pool_labels), the encoder's planes are written from the
 * pooled runs (k_pool_planes), and the encoder's crack and label stages follow for the OUTPUT's shape, the label stage
 * reading the pooled runs.  `flags` must be 0.  FLAT, pin and version 0 streams; signed streams, another factor and
 * flags other than 0 are CKL_ERR_ARG; a stream without voxels becomes the header-only stream of the output's shape,
 * without a device.  A damaged slice fails as in ckl_decompress.  *out is released with ckl_free. */
int ckl_downsample(const uint8_t* buf, uint64_t n, int fx, int fy, int fz, int flags, int markov_model_order, int device,
                   uint8_t** out, uint64_t* out_len);

/* Two streams of one shape merged by a rule on their labels (the reference has none): the stream that ckl_compress gives
 * for the combined volume, written as ckl_erode writes its own (FLAT labels, format version 1, markov_model_order < 0:
 * keep a's, a's fortran_order flag; the crack format is the one the combined volume itself selects).  With a and b the
 * labels of buf_a and buf_b at a voxel, b mattering only as "is it 0":
 *   CKL_COMBINE_OVERLAY      b != 0 ? b : a    the data width is the larger of the two streams'
 *   CKL_COMBINE_KEEP_WHERE   b != 0 ? a : 0    a's data width; b's labels never appear
 *   CKL_COMBINE_DROP_WHERE   b != 0 ? 0 : a    likewise
 * The streams may differ in everything but shape: data width, FLAT or pin labels, format version, crack format, markov
 * order, memory order.  No voxel is decoded and no dense label volume exists: both decoders run up to their run tables
 * on the one device, the words are cut where either stream's row has a break (k_combine_cuts), the rule is evaluated
 * once per cut with one run cursor per stream (k_combine_labels), the encoder's planes are written from those labelled
 * cuts by ckl_downsample's own kernel (k_pool_planes), and the encoder's crack and label stages follow, the label stage
 * reading the cuts.  `flags` must be 0.  Streams of different shapes, signed streams, an unknown rule and flags other
 * than 0 are CKL_ERR_ARG; streams without voxels become the header-only stream of their shape, without a device.  A
 * damaged slice fails as in ckl_decompress, buf_a's first.  *out is released with ckl_free. */
#define CKL_COMBINE_OVERLAY     0
#define CKL_COMBINE_KEEP_WHERE  1   /* mask_by */
#define CKL_COMBINE_DROP_WHERE  2   /* mask_by(invert=True) */
int ckl_combine(const uint8_t* buf_a, uint64_t n_a, const uint8_t* buf_b, uint64_t n_b,
                int rule, int flags /* must be 0 */, int markov_model_order /* -1: a's */, int device,
                uint8_t** out, uint64_t* out_len);

/* An x, y, z box of a stream as a stream of its own (the reference has none; ckl_cutout gives the box as voxels): the
 * stream that ckl_compress gives for the voxels [x0, x1) x [y0, y1) x [z0, z1) of the decoded volume, written as
 * ckl_erode writes its own (FLAT labels, format version 1, markov_model_order < 0: keep the input's, the input's data
 * width and fortran_order flag; the crack format, the stored width and the key widths are the ones the box itself
 * selects).  ckl_crop_boxes gives one stream per box, in order, each exactly what ckl_crop gives for that box, and decodes
 * the stream ONCE for all of them; ckl_crop is ckl_crop_boxes with one box.
 *   boxes     [n_boxes][6]: x0 x1 y0 y1 z0 z1.  Boxes may overlap, repeat and stand in any order.
 *   outs      [n_boxes] streams, each released with ckl_free; out_lens [n_boxes] their lengths
 * Bounds as for ckl_cutout: 0 <= x0 <= x1 <= sx and likewise y and z, else CKL_ERR_ARG with the axis in ckl_last_error;
 * nothing is clamped, and every box is checked before any device work.  A box with an axis of size 0 becomes the
 * header-only stream of its shape, without a device; the box that is the whole volume gives what ckl_recompress gives.
 * n_boxes == 0 is CKL_OK and touches nothing.  `flags` must be 0; flags other than 0 and signed streams are CKL_ERR_ARG.
 * No voxel is decoded and no dense label volume exists, neither the input's nor a box's: one decode session runs up to
 * its run tables over the slices [min z0, max z1) of the boxes with voxels, one label per run is gathered once, and
 * every box then takes a turn: its words are cut where the input row under them has a break (k_crop_cuts), the labels
 * at the cuts are read through the runs (k_crop_labels), the encoder's planes are written from those labelled cuts by
 * ckl_downsample's own kernel (k_pool_planes), and the encoder's crack and label stages follow for the BOX's shape.
 * Boxes of one shape share an encode session.  A damaged slice inside [min z0, max z1) fails as in ckl_decompress,
 * whichever box is asked for; one outside that range is never looked at.  On any error every stream already handed
 * out is freed and all of outs are left null. */
int ckl_crop(const uint8_t* buf, uint64_t n,
             int64_t x0, int64_t x1, int64_t y0, int64_t y1, int64_t z0, int64_t z1,
             int flags /* must be 0 */, int markov_model_order /* -1: the stream's */, int device,
             uint8_t** out, uint64_t* out_len);
int ckl_crop_boxes(const uint8_t* buf, uint64_t n, const int64_t* boxes /* [n_boxes][6]: x0 x1 y0 y1 z0 z1 */, uint64_t n_boxes,
                   int flags /* must be 0 */, int markov_model_order /* -1: the stream's */, int device,
                   uint8_t** outs, uint64_t* out_lens);

/* Native form of crackle.operations.zsplit's range helper (crackle/operations.py:550-623):
 * the stream of slices [z_start, z_end) of a FLAT stream, without decoding (host only).
 * *out is released with ckl_free. */
int ckl_zsplit(const uint8_t* buf, uint64_t n, int64_t z_start, int64_t z_end, uint8_t** out, uint64_t* out_len);

/* Replaces crackle.operations.connected_components (crackle/operations.py:859-934, which decodes
 * slabs, calls the cc3d package and compresses again): the stream in which every 3D-connected piece
 * of a label has an id of its own, 1 .. N in the order of the pieces' first voxels (x fastest, then
 * y, then z); label 0 stays 0.  connectivity is 6, 18 or 26.  The crack codes already hold the
 * 4-connected components of every slice, so the device only links those across rows, diagonals and
 * slices (k_run_links: a union-find over the components) and numbers the sets; z-index, markov
 * model, crack codes and slice crcs are copied, header and label section (uint32, FLAT) are new.
 * component_labels (optional): the original label of component i + 1, as ckl_decoder_label_stats
 * reports labels (sign-extended); n_components (optional): N.  Version 0 streams are refused
 * (CKL_ERR_ARG).  Release *out and *component_labels with ckl_free. */
int ckl_connected_components(
	const uint8_t* buf, uint64_t n, int connectivity, int device,
	uint8_t** out, uint64_t* out_len, uint64_t** component_labels, uint64_t* n_components);

/* The stream `buf` (version 1, FLAT or pin labels) with 2D component i of its slices, in stream order,
 * given the value new_ids[i] (0 .. 2^32 - 1; n_ids must be the stream's component count): data width
 * 4, unsigned, FLAT labels written as labels::encode_flat does (src/labels.hpp:92-155), stored width
 * and key width from the values, everything else copied.  Host only, no device needed: the assembly
 * step of ckl_connected_components, exported so that it can be tested on its own.  *out is released
 * with ckl_free. */
int ckl_relabel_components(const uint8_t* buf, uint64_t n, const uint64_t* new_ids, uint64_t n_ids, uint8_t** out, uint64_t* out_len);

/* Removes the "dust" of a stream (cc3d's dust; the reference has no such function): every voxel of a 3D
 * component (as ckl_connected_components defines them: one label, 6 / 18 / 26 neighbours) with fewer than
 * `threshold` voxels becomes 0.  flags: CKL_DUST_BINARY_IMAGE groups all nonzero voxels into components
 * whatever their labels (survivors keep their own labels), CKL_DUST_INVERT removes the components with
 * `threshold` voxels or more instead.  No voxel is decoded and no crack changes: the device links the 2D
 * components (k_run_links), sums the run lengths per 3D component (k_cc_voxels) and rewrites the labels;
 * the result is a canonical FLAT version 1 stream (unique list ascending without duplicates and without
 * labels that nothing carries any more, 0 added when something was removed, keys and stored width from
 * the new list, is_sorted set) with the input's data width, fortran_order flag, z-index, markov model,
 * crack codes and slice crcs.  Removed components keep their cracks; ckl_recompress removes those.
 * n_removed (optional): the 3D components set to 0.  FLAT and pin streams; version 0 and signed streams
 * are CKL_ERR_ARG; the stream of an empty volume comes back as it is, without a device.  A damaged slice
 * fails as in ckl_decompress.  *out is released with ckl_free. */
#define CKL_DUST_BINARY_IMAGE 1
#define CKL_DUST_INVERT       2
int ckl_dust(const uint8_t* buf, uint64_t n, uint64_t threshold, int connectivity, int flags, int device,
             uint8_t** out, uint64_t* out_len, uint64_t* n_removed /* may be NULL */);

/* Fills the enclosed background voids of a stream (the fill_holes of fill_voids / fastmorph; the reference has no
 * such function).  A hole is a maximal set of voxels with label 0 joined by 6-, 18- or 26-neighbour steps
 * (`connectivity`: the background's).  It is filled with label L when none of its voxels lies on a face of the
 * volume and every face neighbour (the 6 face neighbours, whatever `connectivity` is) of its voxels that is not
 * itself in the hole carries the same label L; every other hole stays 0.  No voxel is decoded and no crack
 * changes: the device links label 0's 2D components (k_run_links), scans the face neighbours of their runs
 * (k_hole_scan) and rewrites the labels; the result is the canonical FLAT version 1 stream ckl_dust describes
 * (label 0 leaves the unique list when every hole was filled) with the input's data width, fortran_order
 * flag, z-index, markov model, crack codes and slice crcs.  Filled holes keep their cracks; ckl_recompress
 * removes those.  n_filled (optional): the holes filled.  FLAT and pin streams; a connectivity other than
 * 6, 18 or 26, version 0 and signed streams are CKL_ERR_ARG; the stream of an empty volume comes back as it
 * is, without a device.  A damaged slice fails as in ckl_decompress.  *out is released with ckl_free. */
int ckl_fill_holes(const uint8_t* buf, uint64_t n, int connectivity, int device,
                   uint8_t** out, uint64_t* out_len, uint64_t* n_filled /* may be NULL */);

/* Host only: the stream `buf` (version 1, unsigned, FLAT or pin labels) with 2D component i of its slices, in
 * stream order, given the label values[i], at the input's data width (n_values must be the stream's component
 * count; a value that does not fit the data width is CKL_ERR_ARG).  The result is the canonical FLAT stream
 * ckl_dust describes: the assembly step of ckl_dust, exported so that it can be tested on its own, and a general
 * "set every component's label" edit.  The stream of an empty volume comes back as it is.  *out is released
 * with ckl_free. */
int ckl_relabel_values(const uint8_t* buf, uint64_t n, const uint64_t* values, uint64_t n_values,
                       uint8_t** out, uint64_t* out_len);

/* crc32c (Castagnoli; src/crc.hpp:51-57) of a host buffer — exported for tests. */
uint32_t ckl_crc32c(const uint8_t* data, uint64_t n);
/* crc32c(A || B) from crc32c(A), crc32c(B) and the byte length of B: lets the ranks of a sharded
 * encode checksum their own parts of the merged label section. */
uint32_t ckl_crc32c_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

#ifdef __cplusplus
}
#endif
#endif /* CRACKLE_AMD_H */
