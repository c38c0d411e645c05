// TEST HARNESS: the stand-alone program.  jpeg_entropy_main <mutations per file> <file>...: every file through the passes of
// the device Huffman decode on the host (emu_jpeg_entropy_dec.cpp) and through the host's decoder; then `mutations` seeded
// mutations of every file's SCAN — flipped bits, overwritten bytes, runs of 0xFF / 0x00 / markers, dropped pieces, truncations
// — through the same, at the call's round cap and at a cap of 2.  Checks per run: "vouched" implies that the host accepts the
// scan and that every coefficient equals the host's.  With the host compiler's sanitizers built in (the Makefile adds them
// where their runtime is installed; the program prints which), an out-of-bounds access or undefined behaviour ends the program;
// a lane that asks for a byte its workgroup would not have staged aborts it.
// jpeg_entropy_main --rounds <file>...: one line per file with its subsequences, launches and the rounds it needs when nothing
// caps them (tools/jpeg_entropy_rounds.py).  jpeg_entropy_main --geometry: the subsequence, the workgroup, the round cap.
#define EMU_JE_NO_SHIM 1
#include "emu_jpeg_entropy_dec.cpp"

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

// One seeded mutation of the bytes from `scan` on
std::vector<uint8_t> mutate(const std::vector<uint8_t> &src, uint32_t scan, Lcg &rng)
{
    std::vector<uint8_t> v = src;
    const uint32_t n = static_cast<uint32_t>(v.size()) - scan;
    if (n == 0) return v;
    switch (rng.below(6)) {
    case 0:
        for (uint32_t k = 1 + rng.below(4); k; --k) v[scan + rng.below(n)] ^= static_cast<uint8_t>(1u << rng.below(8));
        break;
    case 1:
        for (uint32_t k = 1 + rng.below(3); k; --k) v[scan + rng.below(n)] = static_cast<uint8_t>(rng.next());
        break;
    case 2:
        v.resize(scan + rng.below(n));
        break;
    case 3: {
        static const uint8_t values[6] = {0xFF, 0x00, 0xD0, 0xD9, 0x7F, 0xFE};
        const uint32_t from = rng.below(n), len = 1 + rng.below(24);
        for (uint32_t i = from; i < n && i < from + len; ++i) v[scan + i] = values[rng.below(6)];
        break;
    }
    case 4: { // a stuffed pair or a marker at a subsequence's border
        const uint32_t subs = n / pixo_jent::kSubBytes;
        if (subs) {
            const uint32_t at = (1 + rng.below(subs)) * pixo_jent::kSubBytes - rng.below(3);
            if (at + 1 < n) { v[scan + at] = 0xFF; v[scan + at + 1] = rng.below(2) ? 0x00 : static_cast<uint8_t>(rng.next()); }
        }
        break;
    }
    default:
        if (n > 4) { const uint32_t from = rng.below(n - 1), len = 1 + rng.below(16); v.erase(v.begin() + scan + from, v.begin() + scan + std::min(from + len, n)); }
        break;
    }
    return v;
}

} // namespace

int main(int argc, char **argv)
{
    namespace jh = pixo_jdec_host;
    if (argc >= 2 && std::string(argv[1]) == "--geometry") {
        std::printf("sub_bytes=%u group_subs=%u round_cap=%u\n", pixo_jent::kSubBytes, pixo_jent::kGroupSubs, pixo_jent::kRoundCap);
        return 0;
    }
    if (argc < 3) { std::fprintf(stderr, "usage: jpeg_entropy_main <mutations per file> <file>... | --rounds <file>... | --geometry\n"); return 2; }
    const bool rounds_only = std::string(argv[1]) == "--rounds";
    const uint32_t mutations = rounds_only ? 0 : static_cast<uint32_t>(std::atoi(argv[1]));
    uint64_t runs = 0, vouched = 0, redone = 0, host_only = 0, walk_refused = 0, host_refused = 0;
    for (int a = 2; a < argc; ++a) {
        const std::vector<uint8_t> file = read_file(argv[a]);
        if (file.empty()) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        Lcg rng{0x9E3779B97F4A7C15ull ^ static_cast<uint64_t>(a)};
        uint32_t scan = 0;
        for (uint32_t m = 0; m <= mutations; ++m) {
            const std::vector<uint8_t> v = m == 0 ? file : mutate(file, scan, rng);
            // (a copy of exactly the file's bytes on the heap: a read one byte beyond them is seen)
            uint8_t *exact = static_cast<uint8_t *>(std::malloc(v.size() ? v.size() : 1));
            if (!v.empty()) std::memcpy(exact, v.data(), v.size());
            jh::File f;
            std::string msg;
            ++runs;
            if (jh::walk(exact, v.size(), f, &msg) != jh::OK) {
                if (m == 0) { std::fprintf(stderr, "%s refused: %s\n", argv[a], msg.c_str()); return 1; }
                ++walk_refused;
                std::free(exact);
                continue;
            }
            if (m == 0) scan = static_cast<uint32_t>(f.ecs - exact);
            std::vector<int16_t> host(static_cast<size_t>(f.coef_bytes() / 2));
            const bool host_ok = jh::entropy_decode(f, host.data(), &msg) == jh::OK;
            if (!host_ok) ++host_refused;
            if (!pixo_jent::device_takes(f)) {
                ++host_only;
                if (rounds_only) std::printf("%s host\n", argv[a]);
                std::free(exact);
                continue;
            }
            for (const uint32_t cap : {pixo_jent::kRoundCap, 2u}) {
                if (rounds_only && cap == 2u) continue;
                const emu_je::Run r = emu_je::run(f, rounds_only ? 1u << 20 : cap); // (--rounds: what the file needs, uncapped)
                if (rounds_only) {
                    std::printf("%s bytes=%u subs=%u launches=%u rounds=%u vouched=%u why=%u\n", argv[a], static_cast<unsigned>(f.ecs_len), r.status.subs, r.launches,
                                r.status.rounds, r.status.vouched, r.status.why);
                    continue;
                }
                if (!r.status.vouched) { if (cap != 2u) ++redone; continue; }
                if (cap != 2u) ++vouched;
                if (!host_ok || r.coef.size() != host.size() || std::memcmp(r.coef.data(), host.data(), host.size() * 2) != 0) {
                    std::fprintf(stderr, "%s mutation %u cap %u: vouched, but %s\n", argv[a], m, cap, host_ok ? "the coefficients differ from the host's" : "the host refuses the scan");
                    return 1;
                }
            }
            std::free(exact);
        }
    }
    if (rounds_only) return 0;
#if defined(PIXO_SANITIZED)
    const char *how = "sanitized";
#else
    const char *how = "plain";
#endif
    std::printf("%s runs=%llu vouched=%llu redone=%llu host_only=%llu walk_refused=%llu host_refused=%llu\n", how, static_cast<unsigned long long>(runs),
                static_cast<unsigned long long>(vouched), static_cast<unsigned long long>(redone), static_cast<unsigned long long>(host_only),
                static_cast<unsigned long long>(walk_refused), static_cast<unsigned long long>(host_refused));
    return 0;
}
