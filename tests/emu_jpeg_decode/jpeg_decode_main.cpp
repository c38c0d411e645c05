// TEST HARNESS: the stand-alone program.  jpeg_decode_main <mutations per file> <file>...: every file through the library's
// marker walk and entropy decoder and the kernel's code on the host, into buffers of exactly the sizes the library uses; then
// `mutations` seeded mutations of every file — flipped bytes, truncations, swapped markers, overwritten runs — through the
// same.  A run ends with pixels or with a refusal; with the host compiler's sanitizers built in (the Makefile adds them where
// their runtime is installed; the program prints which), a crash, an out-of-bounds access or undefined behaviour ends the
// program instead.  Prints one line of counts; exit status 0 when every run ended.
#include <cstdio>

#include "emu_jpeg_decode.cpp"

namespace {

struct Lcg {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<uint32_t>(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

std::vector<uint8_t> read_file(const char *path)
{
    std::vector<uint8_t> v;
    if (FILE *fp = std::fopen(path, "rb")) {
        uint8_t buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, fp)) > 0;) v.insert(v.end(), buf, buf + n);
        std::fclose(fp);
    }
    return v;
}

// One seeded mutation of a file
std::vector<uint8_t> mutate(const std::vector<uint8_t> &src, Lcg &rng)
{
    std::vector<uint8_t> v = src;
    const uint32_t n = static_cast<uint32_t>(v.size());
    switch (rng.below(6)) {
    case 0: // flip bits of a few bytes anywhere
        for (uint32_t k = 1 + rng.below(4); k; --k) v[rng.below(n)] ^= static_cast<uint8_t>(1u << rng.below(8));
        break;
    case 1: // overwrite a few bytes of the headers
        for (uint32_t k = 1 + rng.below(3); k; --k) v[rng.below(n < 700 ? n : 700)] = static_cast<uint8_t>(rng.next());
        break;
    case 2: // truncate
        v.resize(rng.below(n));
        break;
    case 3: { // swap the codes of two markers
        std::vector<uint32_t> at;
        for (uint32_t i = 0; i + 1 < n; ++i) if (v[i] == 0xFF && v[i + 1] != 0 && v[i + 1] != 0xFF) at.push_back(i + 1);
        if (at.size() >= 2) std::swap(v[at[rng.below(static_cast<uint32_t>(at.size()))]], v[at[rng.below(static_cast<uint32_t>(at.size()))]]);
        break;
    }
    case 4: { // a run of one value (0xFF and 0x00 among them) somewhere
        static const uint8_t values[4] = {0xFF, 0x00, 0xD0, 0x7F};
        const uint32_t from = rng.below(n), len = 1 + rng.below(24);
        for (uint32_t i = from; i < n && i < from + len; ++i) v[i] = values[rng.below(4)];
        break;
    }
    default: // drop a piece
        if (n > 4) { const uint32_t from = rng.below(n - 1), len = 1 + rng.below(16); v.erase(v.begin() + from, v.begin() + (from + len < n ? from + len : n)); }
        break;
    }
    return v;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: jpeg_decode_main <mutations per file> <file>...\n"); return 2; }
    const uint32_t mutations = static_cast<uint32_t>(std::atoi(argv[1]));
    uint64_t runs = 0, decoded = 0, refused = 0;
    for (int a = 2; a < argc; ++a) {
        const std::vector<uint8_t> file = read_file(argv[a]);
        if (file.empty()) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        Lcg rng{0x9E3779B97F4A7C15ull ^ static_cast<uint64_t>(a)};
        for (uint32_t m = 0; m <= mutations; ++m) {
            const std::vector<uint8_t> v = m == 0 ? file : mutate(file, rng);
            // (a copy of exactly the file's bytes on the heap: a read one byte beyond them is seen)
            uint8_t *exact = static_cast<uint8_t *>(std::malloc(v.size() ? v.size() : 1));
            if (!v.empty()) std::memcpy(exact, v.data(), v.size());
            pixo_jdec_host::File f;
            std::string msg;
            uint8_t *block = nullptr;
            const pixo_jdec_host::Kind k = emu_jd::decode(exact, v.size(), m % 3 == 2 ? 3 : m % 3, &block, f, &msg);
            if (m == 0 && k != pixo_jdec_host::OK) { std::fprintf(stderr, "%s refused: %s\n", argv[a], msg.c_str()); return 1; }
            ++runs;
            if (k == pixo_jdec_host::OK) ++decoded; else ++refused;
            std::free(block);
            std::free(exact);
        }
    }
#if defined(PIXO_SANITIZED)
    const char *how = "sanitized";
#else
    const char *how = "plain";
#endif
    std::printf("%s runs=%llu decoded=%llu refused=%llu\n", how, static_cast<unsigned long long>(runs), static_cast<unsigned long long>(decoded),
                static_cast<unsigned long long>(refused));
    return 0;
}
