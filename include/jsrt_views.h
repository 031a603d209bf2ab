/*
 * jsrt_views.h — many cameras of one scene in one call.
 *
 * Reference interface replaced (alitteneker/jsraytracer):
 *   jsrt_camera           <- PerspectiveCamera / DepthOfFieldPerspectiveCamera (src/cameras.js:18-53) as the render path
 *                            reads them: transform, tan_fov, aspect, focus_distance, sensor_size -- the CAMR record of
 *                            include/jsrt_scene.h
 *   jsrt_scene_camera     <- renderer.camera of the loaded scene
 *   jsrt_render_views     <- Camera.setTransform / changeFOV (cameras.js:6-9, 25-28) followed by renderer.render, once
 *                            per view: a second viewpoint without a second scene
 *
 * The one rule: view v of the result is, bit for bit, the frame jsrt_render returns with the same params and the seed
 * view_seeds ? view_seeds[v] : params->seed, for the scene whose CAMR record is cams[v].  The keyed Math.random of a
 * path is keyed (seed of the view, pixel = py * W + px, sample), as in a render: the view index is no part of the
 * key.  A view depends on its camera and seed alone: not on the other views, on nviews or on max_paths.
 *
 * A camera takes tan_fov, not the field of view: the reference stores Math.tan(fov / 2) as V8 computes it, and that
 * double is what parity hangs on.
 *
 * Of params: width, height, spp, max_depth, kind, seed, max_paths, stage_events and mode are honoured, with
 * jsrt_render's defaults from the blob.  Refused (-1, the message names the field): x_offset != 0 or x_delt > 1 (whole
 * frames only), a device_mask other than 0 or the scene's device, nviews < 1, nviews * width * height >= 2^31, a
 * non-affine camera transform, a camera kind that is neither of the two.  There are no progress callbacks.
 *
 * Errors: negative return, message in jsrt_last_error of jsrt.h (-1 arguments, -3 HIP).  JSRT_ABI_VERSION is
 * unchanged: functions are only added.
 */
#ifndef JSRT_VIEWS_H
#define JSRT_VIEWS_H
#include <stddef.h>
#include <stdint.h>

#include "jsrt.h"
#include "jsrt_scene.h" /* JSRT_CAMERA_PERSPECTIVE, JSRT_CAMERA_DOF */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { /* the fields of jsrt_scene.h's CAMR record */
    int32_t kind;         /* JSRT_CAMERA_PERSPECTIVE or JSRT_CAMERA_DOF */
    int32_t pad;
    double transform[16]; /* Mat rows, row-major (row 3 must be 0, 0, 0, 1) */
    double tan_fov, aspect, focus_distance, sensor_size; /* the last two: JSRT_CAMERA_DOF only */
} jsrt_camera;

/* The camera the scene's blob was loaded with. */
int jsrt_scene_camera(jsrt_scene *scene, jsrt_camera *out);

/* nviews frames into host buffers, synchronous.  rgba8: nviews x H x W x 4 bytes, view-major, each view laid out as
 * jsrt_render lays out a full frame; colors_f32 (nullable): nviews x H x W x 4 f32, the colour handed to setColor
 * (alpha 1); view_seeds (nullable): nviews u32, null = params->seed for every view. */
int jsrt_render_views(jsrt_scene *scene, const jsrt_params *params, const jsrt_camera *cams, int32_t nviews,
                      const uint32_t *view_seeds, uint8_t *rgba8, float *colors_f32, jsrt_stats *stats);

/* The same into DEVICE buffers on `hip_stream` (a hipStream_t), asynchronous like jsrt_render_device (with stats, the
 * stream is idle on return).  d_rgba8: nviews x H x W u32 RGBA8, row-major per view (not jsrt_render_device's packed
 * columns); d_colors (nullable): nviews x H x W x 4 f32.  cams and view_seeds are HOST pointers (they are small): the
 * library copies them. */
int jsrt_render_views_device(jsrt_scene *scene, const jsrt_params *params, const jsrt_camera *cams, int32_t nviews,
                             const uint32_t *view_seeds, uint32_t *d_rgba8, float *d_colors, void *hip_stream,
                             jsrt_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
