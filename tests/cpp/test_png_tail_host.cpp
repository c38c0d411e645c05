// The host-only pieces of the PNG tail (pixo_amd/csrc/png_encode_api.cpp: seg_layout, adler_of_chunks, png_head, frame_idats),
// reached by including the translation unit, with a main of its own: nothing here touches a device.  Built with the host
// sanitizers and run by tests/test_png_tail_host.py.
#include "../../pixo_amd/csrc/png_encode_api.cpp"
#include <cstdio>
#include <cstdlib>
static uint32_t adler_ref(const std::vector<uint8_t> &d) { uint64_t a = 1, b = 0; for (uint8_t x : d) { a = (a + x) % 65521; b = (b + a) % 65521; } return (uint32_t)((b << 16) | a); }
int main()
{
    int bad = 0;
    // seg_layout: tables of 1, 3 and 1024 segments, exact heap blocks of n + 1 entries
    for (uint32_t n : {1u, 3u, 1024u}) {
        std::vector<ZSegment> t(n + 1);
        for (uint32_t i = 0; i < n; ++i) t[i] = ZSegment{uint64_t{i} * 70000, 1 + (i * 65535ull) % 200001, 0, 0, 0, 3, 301, 0, 0};
        if (!seg_layout(t.data(), n)) ++bad;
        for (uint32_t i = 0; i < n; ++i) {
            if (t[i + 1].first_chunk - t[i].first_chunk != seg_chunks(t[i].len) || t[i + 1].dst - t[i].dst != seg_dst_bytes(t[i].len) || t[i].dst % 16) ++bad;
            for (uint32_t g = t[i].first_chunk; g < t[i + 1].first_chunk; ++g) if (seg_of_chunk(t.data(), n, g) != i) ++bad;
            if (seg_of_piece(t.data(), n, t[i].first_piece) != i || seg_of_piece(t.data(), n, t[i + 1].first_piece - 1) != i) ++bad;
        }
    }
    { std::vector<ZSegment> t(2); t[0] = ZSegment{0, uint64_t{1} << 47, 0, 0, 0, 0, 0, 0, 0}; if (seg_layout(t.data(), 1)) ++bad; } // pieces past 31 bits: refused
    // adler_of_chunks against the plain definition, lengths around the chunk size
    for (size_t len : {size_t{1}, size_t{65535}, size_t{65536}, size_t{2 * 65535 + 7}, size_t{200000}}) {
        std::vector<uint8_t> d(len);
        uint32_t x = 12345; for (auto &v : d) { x = x * 1103515245u + 12345u; v = (uint8_t)(x >> 16); }
        const uint64_t chunks = pixo_dev::z_chunks(len);
        std::vector<pixo_dev::ZChunkInfo> info(chunks);
        for (uint64_t c = 0; c < chunks; ++c) {
            const size_t c0 = c * 65535, n = std::min<size_t>(65535, len - c0);
            info[c] = {0, 0, 0, 0};
            for (size_t i = 0; i < n; ++i) { info[c].sum_a += d[c0 + i]; info[c].sum_b += (n - i) * (unsigned long long)d[c0 + i]; }
        }
        if (adler_of_chunks(info.data(), chunks, len) != adler_ref(d)) { ++bad; std::printf("adler %zu\n", len); }
    }
    // png_head: gray, and a palette of 256 / 3 entries with tRNS trimmed
    pixo_png_layout lay; std::memset(&lay, 0, sizeof lay); lay.bit_depth = 8;
    if (png_head(7, 9, lay, 0).size() != 8 + 25) ++bad;
    for (uint32_t n : {3u, 256u}) {
        lay.color_type_byte = 3; lay.palette_len = n; lay.has_trns = 1;
        for (uint32_t i = 0; i < n; ++i) { lay.palette[i][0] = i; lay.palette[i][3] = 255 - i; }
        const std::vector<uint8_t> h = png_head(7, 9, lay, n / 2 + 1);
        if (h.size() != 8 + 25 + 12 + 3 * n + 12 + n / 2 + 1) ++bad;
    }
    // frame_idats: streams around the IDAT and piece sizes in exact heap blocks; every chunk's CRC against crc32_bytes
    for (uint64_t sl : {uint64_t{8}, uint64_t{4096}, uint64_t{4097}, uint64_t{262144}, uint64_t{262145}, uint64_t{600001}}) {
        const size_t framed = (size_t)pixo_dev::z_framed_size(sl);
        std::vector<uint8_t> buf(framed + 12, 0xEE);
        const uint64_t idats = (sl + pixo_dev::kIdatBytes - 1) / pixo_dev::kIdatBytes;
        std::vector<uint32_t> crc((sl + 4095) / 4096);
        uint32_t x = 99;
        for (uint64_t s = 0; s < sl; ++s) { x = x * 1103515245u + 12345u; buf[s + 8 + 12 * (s / pixo_dev::kIdatBytes)] = (uint8_t)(x >> 16); }
        for (uint64_t p = 0; p < crc.size(); ++p) { const uint64_t s0 = p * 4096, n = std::min<uint64_t>(4096, sl - s0); crc[p] = crc32_bytes(0, &buf[s0 + 8 + 12 * (s0 / pixo_dev::kIdatBytes)], n); }
        frame_idats(buf.data(), sl, crc.data());
        size_t at = 0;
        for (uint64_t k = 0; k <= idats; ++k) {
            const uint32_t n = (uint32_t(buf[at]) << 24) | (buf[at + 1] << 16) | (buf[at + 2] << 8) | buf[at + 3];
            const uint32_t want = crc32_bytes(0, &buf[at + 4], 4 + n), got = (uint32_t(buf[at + 8 + n]) << 24) | (buf[at + 9 + n] << 16) | (buf[at + 10 + n] << 8) | buf[at + 11 + n];
            if (want != got || std::memcmp(&buf[at + 4], k < idats ? "IDAT" : "IEND", 4)) { ++bad; std::printf("frame %llu chunk %llu\n", (unsigned long long)sl, (unsigned long long)k); }
            at += 12 + n;
        }
        if (at != framed + 12) ++bad;
    }
    std::printf(bad ? "FAILED %d\n" : "all checks passed (%d)\n", bad);
    return bad ? 1 : 0;
}
