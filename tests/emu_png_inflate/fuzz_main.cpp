// TEST HARNESS — a stand-alone program (its own main; built with the host compiler's address and undefined-behaviour
// sanitizers where their runtime exists) that drives the device inflate's walk, compiled for the host, over a corpus of zlib
// streams and over seeded corruptions of them: bit flips, truncations, sizes off by one.  For every case it checks that
//   * the walk ends within the bound png_inflate_math.h states (8 * in_len + expected + 1 loop turns),
//   * nothing outside out[0, produced) is written — guard bytes on both sides and behind `produced` —, produced <= expected,
//   * the reported Adler-32 is that of the bytes produced,
//   * against the host inflate (pixo_amd/csrc/png_inflate.cpp): a stream the batch driver would accept from the device
//     (verdict OK, Adler-32 equal to the stream's last four bytes) is one the host accepts, with equal bytes; and a stream the
//     host accepts is OK on the device or NEEDS_HOST.  (The zlib header is the driver's check: streams that fail it never
//     reach the kernel and are skipped here, after checking that the host refuses them.)
// usage: fuzz_main CORPUS [corruptions per stream]     CORPUS: "PIFZ", u32 count, then per stream u32 len, u64 expected, bytes
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../pixo_amd/csrc/png_inflate.hpp"
#include "emu_png_inflate.hpp"

namespace {

constexpr size_t kGuard = 64;
constexpr uint8_t kFill = 0xA5;
uint64_t g_cases = 0, g_ok = 0, g_failed = 0, g_needs_host = 0, g_skipped = 0;

struct Rng { // xorshift64*
    uint64_t s;
    uint64_t next()
    {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    uint64_t below(uint64_t n) { return n ? next() % n : 0; }
};

bool header_sound(const std::vector<uint8_t> &z)
{
    if (z.size() < 6) return false;
    if ((z[0] & 0x0F) != 8) return false;
    if (((unsigned{z[0]} << 8) | z[1]) % 31 != 0) return false;
    return !(z[1] & 0x20);
}

int fail(const char *what, const std::string &name)
{
    std::fprintf(stderr, "fuzz_main: %s (%s)\n", what, name.c_str());
    return 1;
}

int check(const std::vector<uint8_t> &z, uint64_t expected, const std::string &name)
{
    ++g_cases;
    std::vector<uint8_t> host(expected + 1, 0);
    std::string msg;
    const pixo_inflate::Kind kind = pixo_inflate::inflate_zlib(z.data(), z.size(), host.data(), expected, &msg);
    if (!header_sound(z)) {
        ++g_skipped;
        return kind == pixo_inflate::OK ? fail("the host accepts a stream with a bad zlib header", name) : 0;
    }
    std::vector<uint8_t> block(expected + 2 * kGuard, kFill);
    uint8_t *out = block.data() + kGuard;
    uint64_t produced = 0, turns = 0, bound = 0;
    uint32_t adler = 0;
    const uint32_t verdict = emu_inflate(z.data(), z.size(), out, expected, &produced, &adler, &turns, &bound);
    if (turns > bound) return fail("more loop turns than the stated bound", name);
    if (produced > expected) return fail("produced more than expected", name);
    for (size_t i = 0; i < kGuard; ++i)
        if (block[i] != kFill || block[kGuard + expected + i] != kFill) return fail("a guard byte was written", name);
    // (a produced byte may equal the fill; a byte behind `produced` must still be the fill)
    for (uint64_t i = produced; i < expected; ++i)
        if (out[i] != kFill) return fail("a byte behind `produced` was written", name);
    if (adler != pixo_inflate::adler32(out, produced)) return fail("the Adler-32 is not that of the bytes produced", name);
    if (verdict == pixo_pngi::OK && produced != expected) return fail("OK with a wrong size", name);
    const size_t end = z.size() - 4;
    const uint32_t stored = (uint32_t{z[end]} << 24) | (uint32_t{z[end + 1]} << 16) | (uint32_t{z[end + 2]} << 8) | z[end + 3];
    const bool accepted = verdict == pixo_pngi::OK && adler == stored;
    verdict == pixo_pngi::OK ? ++g_ok : verdict == pixo_pngi::FAILED ? ++g_failed : ++g_needs_host;
    if (accepted) {
        if (kind != pixo_inflate::OK) return fail(("accepted by the device walk, refused by the host: " + msg).c_str(), name);
        if (std::memcmp(out, host.data(), expected) != 0) return fail("bytes differ from the host inflate's", name);
    }
    if (kind == pixo_inflate::OK && !accepted && verdict != pixo_pngi::NEEDS_HOST) return fail("accepted by the host, FAILED on the device walk", name);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) return fail("usage: fuzz_main CORPUS [corruptions per stream]", "arguments");
    const unsigned per_stream = argc > 2 ? static_cast<unsigned>(std::atoi(argv[2])) : 48;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return fail("cannot open the corpus", argv[1]);
    char magic[4];
    uint32_t count = 0;
    if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "PIFZ", 4) != 0 || std::fread(&count, 4, 1, f) != 1) return fail("not a corpus", argv[1]);
    int bad = 0;
    for (uint32_t c = 0; c < count && !bad; ++c) {
        uint32_t len = 0;
        uint64_t expected = 0;
        if (std::fread(&len, 4, 1, f) != 1 || std::fread(&expected, 8, 1, f) != 1) return fail("short corpus", argv[1]);
        std::vector<uint8_t> z(len);
        if (len && std::fread(z.data(), 1, len, f) != len) return fail("short corpus", argv[1]);
        const std::string name = "stream " + std::to_string(c);
        bad |= check(z, expected, name);
        if (expected) bad |= check(z, expected - 1, name + ", expected - 1");
        bad |= check(z, expected + 1, name + ", expected + 1");
        Rng rng{0x9E3779B97F4A7C15ull ^ (uint64_t{c} << 32) ^ len};
        for (unsigned k = 0; k < per_stream && !bad; ++k) {
            std::vector<uint8_t> m = z;
            std::string how;
            if (k % 4 == 3 && m.size() > 6) { // a truncation (the last four bytes that remain are read as the checksum)
                m.resize(6 + rng.below(m.size() - 6));
                how = "truncated to " + std::to_string(m.size());
            } else if (!m.empty()) {
                const unsigned flips = 1 + static_cast<unsigned>(rng.below(3));
                for (unsigned i = 0; i < flips; ++i) {
                    // most flips in the first 64 bytes: block headers and code lengths are where the walk branches
                    const uint64_t at = rng.below(4) ? rng.below(m.size() < 64 ? m.size() : 64) : rng.below(m.size());
                    const unsigned bit = static_cast<unsigned>(rng.below(8));
                    m[at] ^= static_cast<uint8_t>(1u << bit);
                    how += "bit " + std::to_string(at * 8 + bit) + " ";
                }
            }
            bad |= check(m, expected, name + ", " + how);
        }
    }
    std::fclose(f);
    if (bad) return 1;
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
    const char *san = "address,undefined";
#else
    const char *san = "none";
#endif
#else
    const char *san = "none";
#endif
    std::printf("fuzz_main ok: %llu cases (%llu OK, %llu FAILED, %llu NEEDS_HOST, %llu with a bad zlib header), sanitizers: %s\n",
                (unsigned long long)g_cases, (unsigned long long)g_ok, (unsigned long long)g_failed, (unsigned long long)g_needs_host,
                (unsigned long long)g_skipped, san);
    return 0;
}
