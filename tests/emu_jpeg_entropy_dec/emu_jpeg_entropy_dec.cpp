// TEST HARNESS: the device Huffman decode's own code (pixo_amd/csrc/jpeg_entropy_dec_math.h) on the host, pass by pass, with the
// scaffolding of jpeg_entropy_dec.hip restated as loops: a workgroup is a loop over its lanes, a launch a loop over the
// workgroups, the states at the workgroups' borders cross between launches through two arrays written in turn.  Every byte a lane
// asks for is checked against what its workgroup would have staged.  The shim python loads and the stand-alone program
// (jpeg_entropy_main.cpp) both include this file.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pixo_amd/csrc/jpeg_decode_host.cpp"
#include "../../pixo_amd/csrc/jpeg_entropy_dec_host.hpp"

namespace emu_je {

namespace je = pixo_jent;
namespace jh = pixo_jdec_host;

// The scan as a workgroup sees it: bytes [lo, hi) staged, anything else is a bug of the kernel's
struct Staged {
    const uint8_t *ecs;
    uint32_t lo, hi;
    uint32_t operator()(uint32_t i) const
    {
        if (i < lo || i >= hi) { std::fprintf(stderr, "a lane asked for byte %u outside the staged [%u, %u)\n", i, lo, hi); std::abort(); }
        return ecs[i];
    }
};

struct Run {
    je::FileStatus status{};
    uint32_t launches = 0;
    std::vector<int16_t> coef; // the file's coefficients in the layout of jpeg_decode_math.h (vouched)
};

inline Run run(const jh::File &f, uint32_t cap = je::kRoundCap)
{
    Run out;
    je::FileRecord r;
    je::fill_record(f, r);
    // (an exact copy of the scan padded to 16 as the driver uploads it)
    std::vector<uint8_t> scan((f.ecs_len + 15) & ~size_t{15}, 0);
    std::memcpy(scan.data(), f.ecs, f.ecs_len);
    const uint32_t subs = r.subs, groups = r.groups, len = r.ecs_len;
    std::vector<je::State> entry(subs), exit(subs), border[2];
    std::vector<uint32_t> count(subs), first_block(subs);
    border[0].assign(groups + 1, je::kDead);
    border[1].assign(groups + 1, je::kDead);
    const je::State true_state = je::make_state(0, 0, 0);
    je::NoSink none;

    // ---- passes 1 and 2: the cold decode and the hand-over rounds, launch after launch
    uint32_t used = 0, changed = 1;
    for (uint32_t launch = 0; changed && (launch == 0 || used < cap); ++launch) {
        const bool cold = launch == 0;
        const uint32_t budget = cap - used;
        const std::vector<je::State> &in = border[launch & 1];
        std::vector<je::State> &next = border[(launch & 1) ^ 1];
        uint32_t most = 0;
        changed = 0;
        for (uint32_t g = 0; g < groups; ++g) {
            const uint32_t j0 = g * je::kGroupSubs, j1 = std::min(subs, j0 + je::kGroupSubs);
            const Staged by{scan.data(), je::stage_lo(g), je::stage_hi(g, len)};
            const uint32_t limit = std::min(len, by.hi);
            if (cold)
                for (uint32_t j = j0; j < j1; ++j) {
                    entry[j] = j ? je::cold_entry(by, limit, j) : true_state;
                    const je::Exit x = je::decode_sub(by, limit, r, j, entry[j], ~0u, none);
                    exit[j] = x.state; count[j] = x.packed();
                }
            uint32_t rounds = 0, unfinished = 0;
            for (;;) {
                std::vector<uint32_t> need;
                for (uint32_t j = j0; j < j1; ++j) {
                    if (cold && j == j0 && g) continue; // (no border state yet)
                    const je::State pred = j == 0 ? true_state : j == j0 ? in[g] : exit[j - 1];
                    if (pred != entry[j]) need.push_back(j);
                }
                if (need.empty()) break;
                if (rounds == budget) { unfinished = 1; break; }
                std::vector<je::State> preds;
                for (const uint32_t j : need) preds.push_back(j == 0 ? true_state : j == j0 ? in[g] : exit[j - 1]);
                for (size_t n = 0; n < need.size(); ++n) {
                    const uint32_t j = need[n];
                    entry[j] = preds[n];
                    const je::Exit x = je::decode_sub(by, limit, r, j, entry[j], ~0u, none);
                    exit[j] = x.state; count[j] = x.packed();
                }
                ++rounds;
            }
            if (unfinished || (cold ? g + 1 < groups : exit[j1 - 1] != in[g + 1])) ++changed;
            next[g + 1] = exit[j1 - 1];
            most = std::max(most, rounds);
        }
        used += most;
        out.launches = launch + 1;
    }

    // ---- pass 3: verify and place
    je::FileStatus &st = out.status;
    st.subs = subs; st.rounds = used; st.why = je::SHORT;
    uint32_t prefix = 0;
    for (uint32_t j = 0; j < subs; ++j) {
        if (entry[j] != (j ? exit[j - 1] : true_state)) { st.why = je::NOT_SETTLED; break; }
        first_block[j] = prefix;
        const uint32_t clean = count[j] & 0x7FFFFFFFu;
        if (prefix + clean >= r.blocks) { st.why = je::VOUCHED; st.vouched = 1; st.last_sub = j; break; }
        if (exit[j] == je::kDead || (count[j] >> 31)) { st.why = je::CHAIN_DEAD; break; }
        prefix += clean;
    }
    if (!st.vouched) return out;

    // ---- pass 4: write (the staging zeroed first)
    out.coef.assign(static_cast<size_t>(f.coef_bytes() / 2), 0);
    for (uint32_t j = 0; j <= st.last_sub; ++j) {
        const uint32_t g = j / je::kGroupSubs;
        const Staged by{scan.data(), je::stage_lo(g), je::stage_hi(g, len)};
        je::WriteSink sink(r, out.coef.data(), jh::kZigzag, first_block[j]);
        (void)je::decode_sub(by, std::min(len, by.hi), r, j, entry[j], r.blocks - first_block[j], sink);
    }
    // ---- pass 5: the DC differences summed per component in scan order
    for (uint32_t c = 0; c < r.ncomp; ++c) {
        int16_t *plane = out.coef.data() + r.coef_at[c] / 2;
        uint32_t acc = 0;
        for (uint32_t n = 0; n < r.comp_blocks[c]; ++n) {
            int16_t &dc = plane[je::coef_index(je::scan_order_block(r, c, n), 0)];
            acc += static_cast<uint16_t>(dc);
            dc = static_cast<int16_t>(acc);
        }
    }
    return out;
}

} // namespace emu_je

#if !defined(EMU_JE_NO_SHIM)
extern "C" {

// status: 0 decoded, 1 / 2 the walk refused (msg), 3 the host decodes this file from the start.  info[0..5]: vouched, why,
// subsequences, rounds, launches, 1 when the host's entropy decoder accepts the scan.  coef: capacity int16 values for the
// file's coefficients, written when vouched.
int emu_je_run(const uint8_t *file, size_t len, uint32_t cap, int16_t *coef, size_t capacity, uint32_t info[6], char *msg)
{
    pixo_jdec_host::File f;
    std::string m;
    const pixo_jdec_host::Kind k = pixo_jdec_host::walk(file, len, f, &m);
    std::snprintf(msg, 256, "%s", m.c_str());
    if (k != pixo_jdec_host::OK) return static_cast<int>(k);
    std::vector<int16_t> host(static_cast<size_t>(f.coef_bytes() / 2));
    info[5] = pixo_jdec_host::entropy_decode(f, host.data(), &m) == pixo_jdec_host::OK;
    if (!pixo_jent::device_takes(f)) return 3;
    const emu_je::Run r = emu_je::run(f, cap ? cap : pixo_jent::kRoundCap);
    info[0] = r.status.vouched; info[1] = r.status.why; info[2] = r.status.subs; info[3] = r.status.rounds; info[4] = r.launches;
    if (r.status.vouched && capacity >= r.coef.size()) std::memcpy(coef, r.coef.data(), r.coef.size() * 2);
    return 0;
}
// The host decoder's coefficients in the same layout (0: accepted)
int emu_je_host(const uint8_t *file, size_t len, int16_t *coef, size_t capacity)
{
    pixo_jdec_host::File f;
    if (pixo_jdec_host::walk(file, len, f, nullptr) != pixo_jdec_host::OK) return 1;
    std::vector<int16_t> host(static_cast<size_t>(f.coef_bytes() / 2));
    if (pixo_jdec_host::entropy_decode(f, host.data(), nullptr) != pixo_jdec_host::OK) return 2;
    if (capacity >= host.size()) std::memcpy(coef, host.data(), host.size() * 2);
    return 0;
}
size_t emu_je_coef_values(const uint8_t *file, size_t len)
{
    pixo_jdec_host::File f;
    return pixo_jdec_host::walk(file, len, f, nullptr) == pixo_jdec_host::OK ? static_cast<size_t>(f.coef_bytes() / 2) : 0;
}
void emu_je_geometry(uint32_t g[5])
{
    g[0] = pixo_jent::kSubBytes; g[1] = pixo_jent::kGroupSubs; g[2] = pixo_jent::kRoundCap; g[3] = pixo_jent::kMinScanBytes;
    g[4] = static_cast<uint32_t>(sizeof(pixo_jent::FileRecord));
}

} // extern "C"
#endif
