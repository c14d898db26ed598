// Crack codes as packed words: 16 code points of 2 bits in a 32-bit word, code point i of a slice at bits 2 (i mod 16) of
// word i / 16 — the payload's own layout (pack_codepoints, src/crackcodes.hpp:455-496).  The arithmetic k_trail_emit
// (ckl_encode.hip) does on such words, free of anything the device alone has: it compiles as plain C++ as well
// (tests/test_code_words.py checks it there against a byte per code point).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define CKL_HOST_DEVICE __host__ __device__
#else
#define CKL_HOST_DEVICE
#endif

namespace ckl {

// A segment's code points as k_trail_segments keeps them beside its dart: 128 bits, code point j at bit 2 j of q; the
// first len (1 .. 64) are the segment's own (the half of a split segment keeps the whole segment's: a prefix).  Placed so
// that its first code point becomes code point `index` of the slice, they cover the five words out[0 .. 4] from word
// index / 16 on (the return value); words they do not reach come out 0.
CKL_HOST_DEVICE inline uint32_t place_codes128(const uint32_t (&q)[4], uint32_t len, uint32_t index, uint32_t (&out)[5]) {
	uint32_t m[4];
	for (uint32_t j = 0; j < 4; j++) {
		const uint32_t bits = 2u * len > 32u * j ? 2u * len - 32u * j : 0u;      // of word j that belong to the segment
		m[j] = q[j] & (bits >= 32u ? 0xFFFFFFFFu : (1u << bits) - 1u);
	}
	const uint32_t s = 2u * (index & 15u);
	if (s == 0u) { out[0] = m[0]; out[1] = m[1]; out[2] = m[2]; out[3] = m[3]; out[4] = 0u; }
	else {
		out[0] = m[0] << s;
		out[1] = (m[1] << s) | (m[0] >> (32u - s));
		out[2] = (m[2] << s) | (m[1] >> (32u - s));
		out[3] = (m[3] << s) | (m[2] >> (32u - s));
		out[4] = m[3] >> (32u - s);
	}
	return index >> 4;
}

// The difference code of a word of absolute codes: field j becomes (c[j] - c[j - 1]) & 3, where c[-1] is prev_top, the
// last code point of the word in front (0 in front of a slice's first word).  The predecessors are the word moved up by
// one field; the sixteen subtractions share one: the minuend's high bits are set so that no field borrows from its
// neighbour, the subtrahend's are cleared, and the high bit of every difference is put right afterwards.
CKL_HOST_DEVICE inline uint32_t packed_code_diff(uint32_t word, uint32_t prev_top) {
	constexpr uint32_t H = 0xAAAAAAAAu;
	const uint32_t pred = (word << 2) | (prev_top & 3u);
	return ((word | H) - (pred & ~H)) ^ ((word ^ ~pred) & H);
}

}  // namespace ckl
