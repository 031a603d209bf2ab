/*
 * jsrt_color.h — World.color as a batch: the colour of caller-supplied rays.
 *
 * Reference interface replaced (alitteneker/jsraytracer):
 *   jsrt_color[_device] <- World.color(ray, depth) (src/world.js:31-41), the entry every renderer calls once per
 *                          sample with a ray of its camera.  jsrt_render reaches it only with the rays of the blob's
 *                          PerspectiveCamera on its pixel grid; here the host brings the rays: another camera model
 *                          (orthographic, fisheye, panorama), a light probe, a crop, one picked pixel, rays computed
 *                          on the device.
 *   jsrt_camera_rays    <- Camera.getRayForPixel (src/cameras.js:29-52) for every pixel of a frame, with the
 *                          renderer's jitter (src/renderers.js:95-96): the rays jsrt_render itself starts.
 *
 * Math.random is the keyed generator of jsrt.h: the draws of ray i, sample s come from the key
 * (seed, pixel = keys ? keys[i] : i, sample = sample0 + s), and the ray opens the root World.color frame (the first
 * child of the pre-root frame, whose own draws -- jitter, depth of field -- belong to a camera).  So
 * jsrt_color(jsrt_camera_rays(params, s), keys = 0 .. W*H-1, sample0 = s) is, bit for bit, the colour jsrt_render
 * folds into pixel i as its sample s.  A ray's colour depends on its six floats, its key and the sample index only:
 * not on its place in the batch, on the batch's other rays or on max_paths.
 *
 * The root call's minDistance is 0, as a render's; three colour components are returned (the kernels carry three).
 *
 * Errors: negative return, message in jsrt_last_error of jsrt.h (-1 arguments, -3 HIP).  JSRT_ABI_VERSION is
 * unchanged: functions are only added.
 */
#ifndef JSRT_COLOR_H
#define JSRT_COLOR_H
#include <stddef.h>
#include <stdint.h>

#include "jsrt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t max_depth;    /* < 0: the blob's maxRecursionDepth; 0: black (World.color(ray, 0)) */
    uint32_t seed;        /* keyed RNG seed, as jsrt_params.seed */
    uint32_t sample0;     /* first sample index */
    int32_t spp;          /* samples per ray (<= 0: 1); each is its own World.color call */
    int32_t max_paths;    /* batch size in paths (<= 0: library default) */
    int32_t reserved[3];
} jsrt_color_params;

/* out_rgb[3*(i*spp+s)..] = the first three components of World.color(ray_i, max_depth) with Math.random
 * keyed by (seed, pixel = keys ? keys[i] : i, sample = sample0+s).  rays: n x 6 f32 (origin xyz with w = 1,
 * direction xyz with w = 0, as jsrt_cast takes them).  A miss gives World.bg_color.  Host, synchronous. */
int jsrt_color(jsrt_scene *scene, const float *rays, const uint32_t *keys, size_t n, const jsrt_color_params *params,
               float *out_rgb, jsrt_stats *stats);
/* The same on device pointers and a caller stream (hipStream_t), asynchronous like jsrt_render_device (with
 * stats, the stream is idle on return). */
int jsrt_color_device(jsrt_scene *scene, const float *d_rays, const uint32_t *d_keys, size_t n,
                      const jsrt_color_params *params, float *d_out_rgb, void *hip_stream, jsrt_stats *stats);
/* The rays a render with `params` starts for sample `sample`: W*H x 6 f32 in pixel order py*W+px.  Host, synchronous. */
int jsrt_camera_rays(jsrt_scene *scene, const jsrt_params *params, uint32_t sample, float *out_rays);

#ifdef __cplusplus
}
#endif
#endif
