/*
 * jsrt_json.h -- native reader of the reference's Serializer JSON (src/serializer.js).
 *
 *   jsrt_blob_from_json <- Serializer.deserializeJSON(json_txt) (serializer.js:69-71) as the
 *                          dragon_json / toledo_json scenes use it (tests/dragon_json/test.mjs:1-9):
 *                          the text JSON.stringify(new Serializer(test).plain()) wrote
 *                          (tests/test_to_json.js:32-35) becomes the JSRT scene blob of
 *                          include/jsrt_scene.h, byte-identical to the blob
 *                          jsraytracer_amd/js/scene_blob.js exports from the live scene.
 *   jsrt_blob_free       <- (include/jsrt_mesh.h) frees the returned blob.
 *
 * The scene the JSON was written from is restored where the reference's own round trip loses it
 * (SURVEY.md §8(f)3): JSON null is read back as +Infinity in BoxSDF.size, AABB half sizes and
 * refractiveIndexRatio, and as NaN in matrices and in an SDFGeometry's AABB centre (an unbounded box moved
 * by a matrix, geometry.js:94-105; a null half size on such an axis is -Infinity); any other null is an
 * error.  Classes are taken from `_t` (PhongPathTracingMaterial.deserialize would build a
 * FresnelPhongMaterial, materials.js:394-396); and Triangle per-vertex normals / UVs, which Triangle.serialize drops (geometry.js:355-357), come
 * from the `psdata_obj` side-channel: the OBJ text(s) the meshes were loaded from, NUL-separated,
 * matched per triangle on its vertex positions.  NULL / 0: no side-channel (face normals, as the
 * reference renders its deserialized scene).
 *
 * Host-only (no GPU).  Returns 0, or negative with the message in jsrt_last_error of include/jsrt.h;
 * the reference throws strings, e.g. "Attempt to deserialize references out of order"
 * (serializer.js:84).
 */
#ifndef JSRT_JSON_H
#define JSRT_JSON_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int64_t objects;        /* OBJS records written */
    int64_t triangles;      /* TRIS records written */
    int64_t bvh_nodes;      /* BVHN records written */
    int64_t psdata_matched; /* triangles that took normals / UVs from the side-channel */
} jsrt_json_info;

int jsrt_blob_from_json(const char *json, size_t json_len, const char *psdata_obj, size_t psdata_len, void **out_blob,
                        size_t *out_n, jsrt_json_info *info);

#ifdef __cplusplus
}
#endif
#endif
