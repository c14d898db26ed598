// TEST INFRASTRUCTURE: the host-only stages of libcrackle_amd under eight host threads at once, built with
// ThreadSanitizer: ckl_pin_labels_host (HostPool and the "threads of its own" branch beside it), ckl_zsplit /
// ckl_zstack, ckl_header_info_from_bytes, failing calls with ckl_last_error (thread_local), and the result
// blocks' cache (host_out_alloc / host_out_free: without a device the malloc branch and the bookkeeping).
// Every result is compared with what the same call gave on one thread before the others started.
// Built and run by tests/test_sanitizers_cpu.py (CPU only).
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/crackle_amd.h"
#include "../../oracle/ckl_oracle.h"

namespace ckl {
void* host_out_alloc(size_t bytes);
void host_out_free(void* p);
bool host_out_is_pinned(const void* p);
}

static std::atomic<int> fails{0};
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); fails++; } } while (0)

static const int kThreads = 8, kRounds = 6;

static uint32_t mix(uint32_t x) { x ^= x >> 16; x *= 0x45D9F3Bu; x ^= x >> 16; x *= 0x45D9F3Bu; x ^= x >> 16; return x; }

// cells of cx x cy pixels, one label each; every `wobble`-th cell changes its label half-way down z, so that labels
// have one or two components per column and the pin stage has a choice to make.  Hundreds of labels: the per-label
// regions of ckl_pin_labels_host split over several threads (grain 32).
struct Volume {
	int sx, sy, sz;
	std::vector<uint32_t> v, cc, nc;
	std::vector<uint8_t> pins;      // ckl_pin_labels_host's section, single-threaded
};

static Volume cells(int sx, int sy, int sz, int cx, int cy, uint32_t seed, int wobble) {
	Volume vol; vol.sx = sx; vol.sy = sy; vol.sz = sz;
	vol.v.resize(static_cast<size_t>(sx) * sy * sz);
	const int nx = (sx + cx - 1) / cx;
	for (int z = 0; z < sz; z++) for (int y = 0; y < sy; y++) for (int x = 0; x < sx; x++) {
		const uint32_t cell = static_cast<uint32_t>(x / cx + nx * (y / cy));
		uint32_t l = 1 + mix(seed + cell) % 100000;
		if (wobble && cell % wobble == 0 && z >= sz / 2) l = 1 + mix(seed + cell + 7919) % 100000;
		vol.v[x + static_cast<size_t>(sx) * (y + static_cast<size_t>(sy) * z)] = l;
	}
	vol.cc.resize(vol.v.size());
	std::vector<uint64_t> per(sz); uint64_t N = 0;
	CHECK(ckl_oracle_connected_components(vol.v.data(), 4, sx, sy, sz, vol.cc.data(), per.data(), &N) == 0);
	vol.nc.assign(per.begin(), per.end());
	return vol;
}

static bool pin_section(const Volume& vol, std::vector<uint8_t>& out) {
	uint8_t* o = nullptr; uint64_t n = 0;
	const int rc = ckl_pin_labels_host(vol.v.data(), 4, vol.cc.data(), vol.sx, vol.sy, vol.sz, vol.nc.data(), 4, 1, 0, &o, &n);
	if (rc != CKL_OK || !o) return false;
	out.assign(o, o + n);
	ckl_free(o);
	return true;
}

struct Stream {
	std::vector<uint8_t> whole;
	std::vector<std::vector<uint8_t>> parts;      // ckl_zsplit of every slice, single-threaded
	ckl_header_info info = {};
};

static Stream stream_of(const Volume& vol) {
	Stream s;
	unsigned char* out = nullptr; uint64_t n = 0;
	CHECK(ckl_oracle_compress(vol.v.data(), 4, 0, vol.sx, vol.sy, vol.sz, 0, 1, 0, 0, 1, 0, 2, &out, &n) == 0);
	if (out) { s.whole.assign(out, out + n); ckl_oracle_free(out); }
	return s;
}

static bool split_all(const Stream& s, int sz, std::vector<std::vector<uint8_t>>& parts) {
	parts.clear();
	for (int z = 0; z < sz; z++) {
		uint8_t* o = nullptr; uint64_t n = 0;
		if (ckl_zsplit(s.whole.data(), s.whole.size(), z, z + 1, &o, &n) != CKL_OK || !o) return false;
		parts.emplace_back(o, o + n);
		ckl_free(o);
	}
	return true;
}

static bool stack_all(const std::vector<std::vector<uint8_t>>& parts, std::vector<uint8_t>& whole) {
	std::vector<const uint8_t*> ptr; std::vector<uint64_t> len;
	for (auto& p : parts) { ptr.push_back(p.data()); len.push_back(p.size()); }
	uint8_t* o = nullptr; uint64_t n = 0;
	if (ckl_zstack(ptr.data(), len.data(), ptr.size(), &o, &n) != CKL_OK || !o) return false;
	whole.assign(o, o + n);
	ckl_free(o);
	return true;
}

// a call that fails with a text only this thread asks for: a stream cut to `cut` bytes (below a header's 24)
static void fails_with_own_text(const Stream& s, size_t cut) {
	std::vector<uint8_t> t(s.whole.begin(), s.whole.begin() + cut);
	ckl_header_info hi;
	CHECK(ckl_header_info_from_bytes(t.data(), t.size(), &hi) == CKL_ERR_FORMAT);
	const std::string want = "crackle: Input too small to be a valid stream. Bytes: " + std::to_string(cut);
	CHECK(want == ckl_last_error());
	uint8_t* o = nullptr; uint64_t n = 0;
	std::vector<uint8_t> bad(s.whole);
	bad[0] = 'x';
	CHECK(ckl_zsplit(bad.data(), bad.size(), 0, 1, &o, &n) == CKL_ERR_FORMAT);
	CHECK(std::string("crackle: Data stream is not valid. Unable to decompress.") == ckl_last_error());
	CHECK(ckl_header_info_from_bytes(nullptr, 0, &hi) == CKL_ERR_ARG);
	CHECK(std::string("crackle_amd: null argument") == ckl_last_error());
	CHECK(ckl_zsplit(t.data(), t.size(), 0, 1, &o, &n) == CKL_ERR_FORMAT);
	CHECK(want == ckl_last_error());
}

// result blocks of both kinds (below and above the 64 KiB from which the library asks for pinned memory), written,
// read back and released in another order than they were taken
static void churn_blocks(uint32_t seed) {
	static const size_t sizes[] = { 1, 100, 4096, 65535, 65536, 200000, 70000, 17 };
	void* p[8];
	for (int i = 0; i < 8; i++) {
		p[i] = ckl::host_out_alloc(sizes[(i + seed) % 8]);
		CHECK(p[i] != nullptr);
		if (p[i]) memset(p[i], static_cast<int>((seed + i) & 0xFF), sizes[(i + seed) % 8]);
	}
	for (int i = 0; i < 8; i++) {
		const int k = (i * 3 + seed) % 8;
		const size_t n = sizes[(k + seed) % 8];
		const uint8_t* b = static_cast<const uint8_t*>(p[k]);
		CHECK(b && b[0] == ((seed + k) & 0xFF) && b[n - 1] == ((seed + k) & 0xFF));
		(void)ckl::host_out_is_pinned(p[k]);
		ckl::host_out_free(p[k]);
	}
}

int main() {
	// ---- one thread: the inputs and what every call gives
	std::vector<Volume> vols;
	vols.push_back(cells(96, 96, 6, 4, 4, 1, 3));       // 576 cells
	vols.push_back(cells(128, 64, 4, 4, 4, 2, 2));      // 512
	vols.push_back(cells(80, 120, 5, 5, 4, 3, 5));      // 480
	vols.push_back(cells(64, 64, 8, 2, 4, 4, 4));       // 512
	for (Volume& v : vols) CHECK(pin_section(v, v.pins) && !v.pins.empty());
	std::vector<Stream> streams;
	for (const Volume& v : vols) {
		streams.push_back(stream_of(v));
		Stream& s = streams.back();
		CHECK(split_all(s, v.sz, s.parts));
		std::vector<uint8_t> again;
		CHECK(stack_all(s.parts, again) && again == s.whole);
		CHECK(ckl_header_info_from_bytes(s.whole.data(), s.whole.size(), &s.info) == CKL_OK);
		CHECK(s.info.sx == static_cast<uint32_t>(v.sx) && s.info.sz == static_cast<uint32_t>(v.sz));
	}
	churn_blocks(0);
	if (fails) { printf("host_threads: %d failures (before any thread started)\n", fails.load()); return 1; }

	// ---- eight threads on all of it at once, each starting at another volume
	std::atomic<int> ready{0};
	std::vector<std::thread> threads;
	for (int t = 0; t < kThreads; t++) threads.emplace_back([&, t] {
		ready++;
		while (ready.load() < kThreads) std::this_thread::yield();
		for (int r = 0; r < kRounds; r++) {
			const size_t k = static_cast<size_t>(t + r) % vols.size();
			std::vector<uint8_t> pins;
			CHECK(pin_section(vols[k], pins) && pins == vols[k].pins);
			std::vector<std::vector<uint8_t>> parts;
			CHECK(split_all(streams[k], vols[k].sz, parts) && parts == streams[k].parts);
			std::vector<uint8_t> whole;
			CHECK(stack_all(parts, whole) && whole == streams[k].whole);
			ckl_header_info hi = {};
			CHECK(ckl_header_info_from_bytes(streams[k].whole.data(), streams[k].whole.size(), &hi) == CKL_OK);
			CHECK(memcmp(&hi, &streams[k].info, sizeof hi) == 0);
			fails_with_own_text(streams[k], static_cast<size_t>(3 + t));
			churn_blocks(static_cast<uint32_t>(t * kRounds + r));
		}
	});
	for (auto& th : threads) th.join();
	printf("host_threads: %d failures\n", fails.load());
	return fails ? 1 : 0;
}
