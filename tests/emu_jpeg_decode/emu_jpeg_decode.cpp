// TEST HARNESS: JPEG decode on the host — the library's marker walk and entropy decoder (jpeg_decode_host.cpp) and the
// kernel's own code (jpeg_decode_math.h: a workgroup's two phases, lane by lane, tile by tile, over planes of exactly the LDS
// size) compiled for the host.  The shim the tests load, and — included by jpeg_decode_main.cpp — the stand-alone program.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../pixo_amd/csrc/jpeg_decode_host.cpp"

namespace emu_jd {

namespace jd = pixo_jdec;
namespace jh = pixo_jdec_host;

template <int CLS, int FORM> void run_tiles(const jd::Record &r, const uint8_t *coef, uint8_t *out)
{
    std::vector<uint8_t> lds(jd::lds_bytes(CLS)); // (heap: the sanitizer sees an access one byte beyond the planes)
    for (uint32_t tile = 0; tile < r.tiles; ++tile) {
        std::memset(lds.data(), 0xA5, lds.size());
        for (uint32_t lane = 0; lane < jd::kWorkgroup; ++lane) jd::phase_a<CLS>(&r, coef, lds.data(), tile, lane, jd::kWorkgroup);
        for (uint32_t lane = 0; lane < jd::kWorkgroup; ++lane) jd::phase_b<CLS, FORM>(&r, lds.data(), out + r.out_at, tile, lane, jd::kWorkgroup);
    }
}

jd::Record record_of(const jh::File &f)
{
    jd::Record r;
    std::memset(&r, 0, sizeof r);
    for (uint32_t c = 0; c < f.ncomp; ++c) {
        r.coef_at[c] = f.plane_at(c);
        std::memcpy(r.q[c], f.q[f.comp[c].tq], sizeof r.q[c]);
    }
    r.width = f.width; r.height = f.height; r.mcus_x = f.mcus_x; r.mcus_y = f.mcus_y;
    r.tiles_x = jd::tiles_x_of(f.mcus_x);
    r.tiles = r.tiles_x * jd::tiles_y_of(f.mcus_y);
    return r;
}

// A whole file -> pixels in a block of exactly misalign + the image's bytes (16-byte aligned before `misalign`).  The caller frees *block.
jh::Kind decode(const uint8_t *file, size_t len, uint32_t misalign, uint8_t **block, jh::File &f, std::string *msg)
{
    *block = nullptr;
    jh::Kind k = jh::walk(file, len, f, msg);
    if (k != jh::OK) return k;
    void *coef = nullptr;
    if (posix_memalign(&coef, 16, static_cast<size_t>(f.coef_bytes()) + 16)) return jh::INVALID;
    k = jh::entropy_decode(f, static_cast<int16_t *>(coef), msg);
    if (k != jh::OK) { std::free(coef); return k; }
    void *mem = nullptr;
    if (posix_memalign(&mem, 16, misalign + static_cast<size_t>(f.pixel_bytes()) + (f.pixel_bytes() ? 0 : 1))) { std::free(coef); return jh::INVALID; }
    uint8_t *out = static_cast<uint8_t *>(mem) + misalign;
    const jd::Record r = record_of(f);
    const uint8_t *c8 = static_cast<const uint8_t *>(coef);
    if (r.tiles) {
        const bool aligned = misalign % 16 == 0;
#define EMU_JD_GO(C) if (aligned) run_tiles<C, jd::F_ALIGNED>(r, c8, out); else run_tiles<C, jd::F_BYTES>(r, c8, out)
        switch (f.cls) {
        case jd::C_GRAY: EMU_JD_GO(jd::C_GRAY); break;
        case jd::C_444: EMU_JD_GO(jd::C_444); break;
        case jd::C_422: EMU_JD_GO(jd::C_422); break;
        default: EMU_JD_GO(jd::C_420); break;
        }
#undef EMU_JD_GO
    }
    std::free(coef);
    *block = static_cast<uint8_t *>(mem);
    return jh::OK;
}

} // namespace emu_jd

extern "C" {

// 0: `out` holds the pixels (capacity >= their bytes); 1 / 2: refused (Invalid / Unsupported), msg (256 bytes) says why; 3: capacity
int emu_jd_decode(const uint8_t *file, size_t len, uint32_t misalign, uint8_t *out, size_t capacity, uint32_t *width, uint32_t *height, uint32_t *color_type,
                  char *msg)
{
    pixo_jdec_host::File f;
    std::string why;
    uint8_t *block = nullptr;
    const pixo_jdec_host::Kind k = emu_jd::decode(file, len, misalign, &block, f, &why);
    std::strncpy(msg, why.c_str(), 255);
    msg[255] = 0;
    if (k != pixo_jdec_host::OK) return k;
    *width = f.width; *height = f.height; *color_type = f.color_type();
    const bool fits = capacity >= f.pixel_bytes();
    if (fits) std::memcpy(out, block + misalign, static_cast<size_t>(f.pixel_bytes()));
    std::free(block);
    return fits ? 0 : 3;
}

// 1: every dequantised block of the file lies inside jpeg_decode_math.h's 32-bit bound; 0: one does not; -1: refused
int emu_jd_within_bound(const uint8_t *file, size_t len)
{
    namespace jh = pixo_jdec_host;
    jh::File f;
    if (jh::walk(file, len, f, nullptr) != jh::OK) return -1;
    std::vector<int16_t> coef(static_cast<size_t>(f.coef_bytes() / 2) + 1);
    if (jh::entropy_decode(f, coef.data(), nullptr) != jh::OK) return -1;
    for (uint32_t c = 0; c < f.ncomp; ++c) {
        const int16_t *plane = coef.data() + f.plane_at(c) / 2;
        for (uint64_t b = 0; b < static_cast<uint64_t>(f.blocks_w(c)) * f.blocks_h(c); ++b) {
            int32_t d[64];
            for (uint32_t n = 0; n < 64; ++n) d[n] = static_cast<int32_t>(plane[pixo_jdec::coef_index(b, n)]) * f.q[f.comp[c].tq][n];
            if (!pixo_jdec::within_bound(d)) return 0;
        }
    }
    return 1;
}

uint32_t emu_jd_record_bytes(void) { return sizeof(pixo_jdec::Record); }
uint32_t emu_jd_lds_bytes(int cls) { return cls == 0 ? pixo_jdec::lds_bytes(0) : cls == 1 ? pixo_jdec::lds_bytes(1) : cls == 2 ? pixo_jdec::lds_bytes(2) : pixo_jdec::lds_bytes(3); }

} // extern "C"
