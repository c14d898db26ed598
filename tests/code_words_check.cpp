// Stand-alone check of crackle_amd/csrc/ckl_code_words.hpp on the host (built and run by tests/test_code_words.py):
// both helpers against a byte per code point.
#include "ckl_code_words.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

int main() {
	long checks = 0;
	// place_codes128: every length 1 .. 64 at every alignment (and a few word offsets), OR-ed into words that hold other
	// code points already, as k_trail_emit does
	for (uint32_t len = 1; len <= 64; len++) {
		for (uint32_t index = 0; index < 16 * 3; index++) {
			for (int rep = 0; rep < 4; rep++) {
				std::vector<uint8_t> codes(len);
				for (auto& c : codes) c = static_cast<uint8_t>(rnd() & 3u);
				uint32_t q[4] = { 0, 0, 0, 0 };
				for (uint32_t j = 0; j < len; j++) q[j >> 4] |= static_cast<uint32_t>(codes[j]) << (2 * (j & 15));
				if (rep & 1) for (uint32_t j = len; j < 64; j++) q[j >> 4] |= (rnd() & 3u) << (2 * (j & 15));      // the half of a split segment: the other half's code points behind its own
				const uint32_t total = 16 * 9;
				std::vector<uint8_t> want(total, 0);
				std::vector<uint32_t> words(total / 16, 0);
				// neighbours in front and behind, placed bytewise
				for (uint32_t g = 0; g < total; g++) {
					if (g >= index && g < index + len) want[g] = codes[g - index];
					else { want[g] = static_cast<uint8_t>(rnd() & 3u); words[g >> 4] |= static_cast<uint32_t>(want[g]) << (2 * (g & 15)); }
				}
				uint32_t out[5];
				const uint32_t w = ckl::place_codes128(q, len, index, out);
				if (w != index / 16) { printf("place_codes128: first word %u for index %u\n", w, index); return 1; }
				const uint32_t last = (index + len - 1) / 16;
				for (uint32_t j = 0; j < 5; j++) {
					if (w + j > last && out[j]) { printf("place_codes128: len %u index %u writes word %u behind its last\n", len, index, j); return 1; }
					words[w + j] |= out[j];
				}
				for (uint32_t g = 0; g < total; g++) {
					if (((words[g >> 4] >> (2 * (g & 15))) & 3u) != want[g]) { printf("place_codes128: len %u index %u code %u\n", len, index, g); return 1; }
					checks++;
				}
			}
		}
	}
	// packed_code_diff: random words behind every top code of the word in front
	for (uint32_t prev_top = 0; prev_top < 4; prev_top++) {
		for (int rep = 0; rep < 20000; rep++) {
			uint32_t word = rnd();
			if (rep == 0) word = 0u;
			if (rep == 1) word = 0xFFFFFFFFu;
			if (rep == 2) word = 0xAAAAAAAAu;
			if (rep == 3) word = 0x55555555u;
			if (rep == 4) word = 0xCCCCCCCCu;      // 0, 3, 0, 3: every field borrows or carries against its neighbour
			if (rep == 5) word = 0x33333333u;
			uint32_t want = 0, prev = prev_top;
			for (uint32_t j = 0; j < 16; j++) {
				const uint32_t c = (word >> (2 * j)) & 3u;
				want |= ((c - prev) & 3u) << (2 * j);
				prev = c;
			}
			const uint32_t got = ckl::packed_code_diff(word, prev_top);
			if (got != want) { printf("packed_code_diff(%08x, %u) = %08x, want %08x\n", word, prev_top, got, want); return 1; }
			checks++;
		}
	}
	// a whole string of random length: words chained through their top codes
	for (uint32_t n = 1; n <= 64; n++) {
		for (int rep = 0; rep < 50; rep++) {
			std::vector<uint8_t> codes(n);
			for (auto& c : codes) c = static_cast<uint8_t>(rnd() & 3u);
			std::vector<uint32_t> words((n + 15) / 16, 0);
			for (uint32_t g = 0; g < n; g++) words[g >> 4] |= static_cast<uint32_t>(codes[g]) << (2 * (g & 15));
			for (uint32_t w = 0; w < words.size(); w++) {
				uint32_t enc = ckl::packed_code_diff(words[w], w ? words[w - 1] >> 30 : 0u);
				for (uint32_t j = 0; j < 16 && 16 * w + j < n; j++) {
					const uint32_t g = 16 * w + j;
					const uint32_t want = (codes[g] - (g ? codes[g - 1] : 0u)) & 3u;
					if (((enc >> (2 * j)) & 3u) != want) { printf("string of %u: code %u\n", n, g); return 1; }
					checks++;
				}
			}
		}
	}
	printf("ok %ld\n", checks);
	return 0;
}
