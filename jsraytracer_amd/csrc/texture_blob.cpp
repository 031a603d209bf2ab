// texture_blob.cpp — jsrt_blob_set_texture (include/jsrt_texture.h): an MCOL record of a JSRT blob turned into a
// texture.  Host-only.  The blob is rewritten section by section in its own order; TEXR / TEXL are appended when the
// blob had none.
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "../../include/jsrt_scene.h"
#include "../../include/jsrt_texture.h"

namespace jsrt {
int record_error(int code, const std::string &m);  // capi.cpp (jsrt_last_error)
}

extern "C" int jsrt_blob_set_texture(const void *blob, size_t n, int32_t mcolor_index, const uint8_t *rgba8, int32_t width,
                                     int32_t height, int32_t mode, int32_t clamp_u, int32_t clamp_v, void **out_blob,
                                     size_t *out_n) {
    using jsrt::record_error;
    if (!out_blob || !out_n) return record_error(-1, "out_blob / out_n is NULL");
    *out_blob = nullptr;
    *out_n = 0;
    if (!blob || n < sizeof(jsrt_blob_header)) return record_error(-1, "blob too small");
    if (width < 1 || height < 1) return record_error(-1, "texture width and height must be at least 1");
    if (mode != JSRT_TEX_BILINEAR && mode != JSRT_TEX_NEAREST) return record_error(-1, "unsupported texture mode");
    if (!rgba8) return record_error(-1, "rgba8 is NULL");
    const uint8_t *b = static_cast<const uint8_t *>(blob);
    jsrt_blob_header h;
    memcpy(&h, b, sizeof h);
    if (h.magic != JSRT_MAGIC || h.version != JSRT_VERSION) return record_error(-1, "not a JSRT v1 blob");
    if (sizeof h + (uint64_t)h.n_sections * sizeof(jsrt_section) > n) return record_error(-1, "truncated section table");
    try {
        std::vector<jsrt_section> secs(h.n_sections);
        std::vector<std::vector<uint8_t>> data(h.n_sections);
        int mcol = -1, texr = -1, texl = -1;
        for (uint32_t i = 0; i < h.n_sections; ++i) {
            memcpy(&secs[i], b + sizeof h + i * sizeof(jsrt_section), sizeof(jsrt_section));
            const jsrt_section &s = secs[i];
            if (s.offset > n || s.bytes > n - s.offset) return record_error(-1, "section out of range");
            data[i].assign(b + s.offset, b + s.offset + s.bytes);
            if (s.tag == JSRT_SEC_MCOLOR) mcol = (int)i;
            if (s.tag == JSRT_SEC_TEXTURE) texr = (int)i;
            if (s.tag == JSRT_SEC_TEXEL) texl = (int)i;
        }
        if (mcol < 0 || data[mcol].size() != (size_t)secs[mcol].count * sizeof(jsrt_rec_mcolor))
            return record_error(-1, "blob has no material colours");
        if (mcolor_index < 0 || (uint32_t)mcolor_index >= secs[mcol].count)
            return record_error(-1, "material colour " + std::to_string(mcolor_index) + " is out of range");
        auto section = [&](int &at, uint32_t tag) {
            if (at >= 0) return;
            at = (int)secs.size();
            secs.push_back(jsrt_section{tag, 0, 0, 0});
            data.emplace_back();
        };
        section(texr, JSRT_SEC_TEXTURE);
        section(texl, JSRT_SEC_TEXEL);
        if (data[texr].size() != (size_t)secs[texr].count * sizeof(jsrt_rec_texture) || data[texl].size() != secs[texl].count)
            return record_error(-1, "bad texture section size");
        const uint64_t bytes = (uint64_t)width * (uint64_t)height * 4;
        const uint64_t at = ((uint64_t)data[texl].size() + 3) & ~(uint64_t)3;  // descriptors point at 4-byte boundaries
        if (at + bytes > UINT32_MAX) return record_error(-1, "more than 4 GiB of texels");
        data[texl].resize((size_t)at, 0);
        data[texl].insert(data[texl].end(), rgba8, rgba8 + bytes);
        secs[texl].count = (uint32_t)data[texl].size();
        jsrt_rec_texture t;
        memset(&t, 0, sizeof t);
        t.width = (uint32_t)width;
        t.height = (uint32_t)height;
        t.mode = (uint32_t)mode;
        t.clamp_u = clamp_u ? 1u : 0u;
        t.clamp_v = clamp_v ? 1u : 0u;
        t.offset = at;
        const uint8_t *tp = reinterpret_cast<const uint8_t *>(&t);
        data[texr].insert(data[texr].end(), tp, tp + sizeof t);
        jsrt_rec_mcolor r;
        memset(&r, 0, sizeof r);
        r.kind = JSRT_MC_TEXTURE;
        r.a = (int32_t)secs[texr].count++;
        r.b = -1;
        memcpy(data[mcol].data() + (size_t)mcolor_index * sizeof r, &r, sizeof r);

        const size_t hdr = sizeof h + secs.size() * sizeof(jsrt_section);
        size_t off = (hdr + 7) & ~(size_t)7, total = off;
        for (const auto &d : data) total += (d.size() + 7) & ~(size_t)7;
        uint8_t *out = static_cast<uint8_t *>(calloc(total, 1));
        if (!out) return record_error(-4, "out of host memory");
        h.n_sections = (uint32_t)secs.size();
        memcpy(out, &h, sizeof h);
        for (size_t i = 0; i < secs.size(); ++i) {
            secs[i].offset = off;
            secs[i].bytes = data[i].size();
            memcpy(out + sizeof h + i * sizeof(jsrt_section), &secs[i], sizeof(jsrt_section));
            if (!data[i].empty()) memcpy(out + off, data[i].data(), data[i].size());
            off += (data[i].size() + 7) & ~(size_t)7;
        }
        *out_blob = out;
        *out_n = total;
        return 0;
    } catch (const std::bad_alloc &) {
        return record_error(-4, "out of host memory");
    }
}
