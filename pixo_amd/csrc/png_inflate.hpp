// png_inflate.hpp — the host inflate of the PNG decoder (png_inflate.cpp): zlib stream in, at most `expected` bytes out.
// No HIP headers: it compiles and runs without the library (a stand-alone program can drive it).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace pixo_inflate {

enum Kind : int { OK = 0, INVALID = 1, UNSUPPORTED = 2 }; // Error::InvalidDecode / Error::UnsupportedDecode (src/error.rs:44-47)

// inflate_zlib_with_size(data, Some(expected)) (src/decode/inflate.rs:294-352) into out[0, expected): the reference's checks in
// its order and with its messages (*msg: the text behind "Decode error: " / "Unsupported: ").  Never writes past `expected`
// bytes: what a stream makes beyond them is kept only as far as later matches can reach (32 KiB), checksummed and counted, so
// that the Adler-32 and size errors read as the reference's.  The Adler-32 is read from the last four bytes of `data`.
Kind inflate_zlib(const uint8_t *data, size_t len, uint8_t *out, size_t expected, std::string *msg);

uint32_t adler32(const uint8_t *data, size_t len, uint32_t start = 1);

} // namespace pixo_inflate
