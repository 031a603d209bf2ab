/*
 * jsrt_texture.h — textures for a JSRT scene blob (include/jsrt_scene.h).  Host-only (never touches the GPU).
 *
 * Reference interface replaced (alitteneker/jsraytracer):
 *   jsrt_blob_set_texture <- new TextureMaterialColor(imgdata, mode, clampU, clampV) (src/materials.js:78-87) put in
 *                            the place of an existing MaterialColor: the way to texture a scene that came from the
 *                            Serializer-JSON reader (jsrt_json.h) or the OBJ ingest (jsrt_mesh.h), neither of which
 *                            can carry one.  (A live reference scene graph exports its textures itself:
 *                            jsraytracer_amd/js/scene_blob.js.)
 *
 * The returned blob is the input with MCOL record `mcolor_index` turned into a texture (JSRT_MC_TEXTURE) over a
 * new TEXR descriptor, its texels appended to TEXL; every material and wrapper that referred to that record now
 * reads the texture.  Whether the slots it sits in accept a texture is decided when the scene is created
 * (jsrt_scene_create), not here.
 *
 * Errors: negative return, message in jsrt_last_error of jsrt.h.
 */
#ifndef JSRT_TEXTURE_H
#define JSRT_TEXTURE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* rgba8: width * height * 4 bytes, ImageData.data order (RGBA, row-major, top row first).  mode: 0 bilinear,
 * 1 nearest (JSRT_TEX_*).  clamp_u / clamp_v: non-zero = Math.clamp(c, 0, 1), zero = wrap.  Returns 0 and a
 * malloc'd blob in *out_blob / *out_n (free with jsrt_blob_free of jsrt_mesh.h), or negative. */
int jsrt_blob_set_texture(const void *blob, size_t n, int32_t mcolor_index, const uint8_t *rgba8, int32_t width,
                          int32_t height, int32_t mode, int32_t clamp_u, int32_t clamp_v, void **out_blob, size_t *out_n);

#ifdef __cplusplus
}
#endif
#endif
