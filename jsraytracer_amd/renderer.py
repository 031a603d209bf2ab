"""Host-side mirror of the reference's renderer interface, backed by the HIP library.

Reference: src/renderers.js (SimpleRenderer.render :10-41, IncrementalMultisamplingRenderer.render
:70-117), src/pixelbuffer.js (PixelBuffer :1-50), src/worker.js (:17-40).  Same names, argument
meaning and error behaviour: ``render(img, timelimit=0, callback=False, x_offset=0, x_delt=1)``
fills ``img``'s RGBA8 bytes for the columns px = x_offset, x_offset + x_delt, ... and calls
``callback({"pass": p, "completion": c})`` no more often than every ``timelimit`` ms.
"""
import ctypes

import numpy as np

from . import _native
from ._native import JsrtError, Params, Stats, check

RENDERER_KINDS = {"SimpleRenderer": 0, "IncrementalMultisamplingRenderer": 1, "RandomMultisamplingRenderer": 2}
MODE_STRICT, MODE_FAST = 0, 1  # include/jsrt.h JSRT_MODE_*: numeric modes; only strict is built
MODES = {"strict": MODE_STRICT, "fast": MODE_FAST}


def mode_code(mode):
    """None / "strict" / "fast" / an int -> JSRT_MODE_* (the library refuses what it does not build)."""
    if mode is None:
        return MODE_STRICT
    if isinstance(mode, str):
        if mode not in MODES:
            raise JsrtError(f"unknown numeric mode {mode!r}")
        return MODES[mode]
    return int(mode)


class PixelBuffer:
    """pixelbuffer.js:1-50 — RGBA8 image (ImageData-like) with the reference's setColor rules."""

    def __init__(self, width, height=None):
        if isinstance(width, np.ndarray):
            self.imgdata = width
        else:
            self.imgdata = np.zeros((height, width, 4), np.uint8)  # new ImageData: zero-filled

    def width(self):
        return self.imgdata.shape[1]

    def height(self):
        return self.imgdata.shape[0]

    def coord(self, x, y):
        return y * (self.width() * 4) + x * 4

    def getColor(self, x, y):
        return self.imgdata[y, x].astype(np.float64) / 255


CAMERA_PERSPECTIVE, CAMERA_DOF = 0, 1  # include/jsrt_scene.h JSRT_CAMERA_*
_CAMR = 0x524D4143  # 'CAMR'
_CAMR_FMT = "<II16d4d"  # jsrt_rec_camera: kind, pad, transform (Mat rows), tan_fov, aspect, focus_distance, sensor_size


class Camera:
    """The camera of one view (include/jsrt_views.h jsrt_camera; cameras.js:18-53 as the render path reads it): kind
    (CAMERA_PERSPECTIVE / CAMERA_DOF), transform (4 x 4 float64, Mat rows; row 3 must be 0, 0, 0, 1), tan_fov, aspect,
    and for CAMERA_DOF focus_distance and sensor_size.  It holds tan_fov, not the field of view: the reference keeps
    Math.tan(fov / 2) as V8 computed it, and a frame is bit-exact only with that double."""

    def __init__(self, transform, tan_fov, aspect, kind=CAMERA_PERSPECTIVE, focus_distance=0.0, sensor_size=0.0):
        self.transform = np.array(transform, np.float64).reshape(4, 4)
        self.tan_fov, self.aspect = float(tan_fov), float(aspect)
        self.kind = int(kind)
        self.focus_distance, self.sensor_size = float(focus_distance), float(sensor_size)

    @classmethod
    def from_fov(cls, fov, aspect, transform, kind=CAMERA_PERSPECTIVE, focus_distance=0.0, sensor_size=0.0):
        """PerspectiveCamera(fov, aspect, transform) with tan_fov = math.tan(fov / 2).  That is the C library's tan,
        not pinned to V8's Math.tan: the two may differ in the last bit.  Where a frame must match the reference bit
        for bit, pass the reference's own tan_fov to Camera(...) instead."""
        import math
        return cls(transform, math.tan(fov / 2), aspect, kind, focus_distance, sensor_size)

    def replace(self, **kw):
        """A copy with some fields replaced."""
        d = dict(transform=self.transform, tan_fov=self.tan_fov, aspect=self.aspect, kind=self.kind,
                 focus_distance=self.focus_distance, sensor_size=self.sensor_size)
        d.update(kw)
        return Camera(**d)

    def _rec(self):
        t = (ctypes.c_double * 16)(*self.transform.reshape(-1).tolist())
        return _native.CameraRec(self.kind, 0, t, self.tan_fov, self.aspect, self.focus_distance, self.sensor_size)

    @classmethod
    def _from_rec(cls, r):
        return cls(np.array(list(r.transform), np.float64), r.tan_fov, r.aspect, r.kind, r.focus_distance, r.sensor_size)

    def __eq__(self, other):
        import struct
        return isinstance(other, Camera) and struct.pack(_CAMR_FMT, *self._fields()) == struct.pack(_CAMR_FMT, *other._fields())

    __hash__ = None

    def _fields(self):
        return [self.kind & 0xFFFFFFFF, 0] + self.transform.reshape(-1).tolist() + \
            [self.tan_fov, self.aspect, self.focus_distance, self.sensor_size]

    def __repr__(self):
        return (f"Camera(kind={self.kind}, tan_fov={self.tan_fov!r}, aspect={self.aspect!r}, "
                f"focus_distance={self.focus_distance!r}, sensor_size={self.sensor_size!r}, "
                f"transform={self.transform.tolist()!r})")


def _camera_section(blob):
    import struct
    magic, version, nsec, _ = struct.unpack_from("<4I", blob, 0)
    if magic != 0x5452534A or version != 1:
        raise JsrtError("not a JSRT v1 scene blob")
    for i in range(nsec):
        tag, count, off, nbytes = struct.unpack_from("<IIQQ", blob, 16 + 24 * i)
        if tag == _CAMR:
            if count != 1 or nbytes != struct.calcsize(_CAMR_FMT) or off + nbytes > len(blob):
                raise JsrtError("scene blob's CAMR section is not one 168-byte camera record")
            return off
    raise JsrtError("scene blob has no camera record")


def blob_camera(blob):
    """The Camera of a scene blob's CAMR record (host-only)."""
    import struct
    f = struct.unpack_from(_CAMR_FMT, blob, _camera_section(blob))
    return Camera(np.array(f[2:18], np.float64), f[18], f[19], f[0], f[20], f[21])


def with_camera(blob, camera):
    """A copy of `blob` with its CAMR record overwritten by `camera`: the scene a view of Scene.render_views is, by
    definition, a render of.  Host-only; the blob's own camera round-trips to the identical blob.  Raises JsrtError for a
    blob without a well-formed CAMR section."""
    import struct
    blob = bytes(blob)
    off = _camera_section(blob)
    rec = struct.pack(_CAMR_FMT, *camera._fields())
    return blob[:off] + rec + blob[off + len(rec):]


class Scene:
    """A JSRT scene blob (include/jsrt_scene.h) uploaded to one HIP device."""

    def __init__(self, blob, device=0):
        L = _native.lib()
        if L.jsrt_device_count() <= 0:
            raise JsrtError("no HIP device visible: the MI355X renderer has no CPU fallback")
        self._blob = bytes(blob)
        h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(self._blob, len(self._blob))
        check(L.jsrt_scene_create(buf, len(self._blob), device, ctypes.byref(h)), "jsrt_scene_create")
        self._h = h
        self.device = device

    def cast(self, rays, min_dist=0.0, max_dist=float("inf"), intersect_transparent=True):
        """World.cast (world.js:28-30) of rays (n x 6 f32: origin xyz w=1, direction xyz w=0) on the
        device: (distance f64, hit Primitive's OBJS index i32, -1 none) per ray."""
        import numpy as np
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = len(rays)
        t = np.empty(n, np.float64)
        obj = np.empty(n, np.int32)
        check(_native.lib().jsrt_cast(self._h, rays.ctypes.data, n, min_dist, max_dist, int(bool(intersect_transparent)),
                                      t.ctypes.data, obj.ctypes.data), "jsrt_cast")
        return t, obj

    CAST_PATHS = {"any": 1, "any_masked": 2, "any_node": 3, "persistent": 4, "persistent_any": 5}

    def cast_path(self, rays, min_dist=0.0, max_dist=float("inf"), intersect_transparent=True, path="any"):
        """The rays of cast() through another of the render's casts (include/jsrt.h jsrt_cast_path): "any" (the
        shadow kernels' any-hit cast), "any_masked" (the same under the wave's shadow-root mask: segments from hit
        points to light sample points, a wave's 64 origins in one grid cell), "any_node" (groups of 4 rays sharing an origin; a shadowed ray reads
        obj -2, t NaN), "persistent" / "persistent_any" (the SDF marches).  (distance, OBJS index) as cast();
        JsrtError when the scene's kernel profile has no such path."""
        import numpy as np
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = len(rays)
        t = np.empty(n, np.float64)
        obj = np.empty(n, np.int32)
        check(_native.lib().jsrt_cast_path(self._h, rays.ctypes.data, n, min_dist, max_dist, int(bool(intersect_transparent)),
                                           self.CAST_PATHS[path], t.ctypes.data, obj.ctypes.data), "jsrt_cast_path")
        return t, obj

    def material_data(self, rays):
        """World.color(ray, 1) up to Material.color (include/jsrt.h jsrt_material_data): dict of t, obj,
        normal (n x 4), position (n x 4), uv (n x 3), bary (n x 3), basecolor (n x 3); NaN = absent."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = len(rays)
        out = {"t": np.empty(n, np.float64), "obj": np.empty(n, np.int32)}
        for k, w in (("normal", 4), ("position", 4), ("uv", 3), ("bary", 3), ("basecolor", 3)):
            out[k] = np.empty((n, w), np.float32)
        check(_native.lib().jsrt_material_data(self._h, rays.ctypes.data, n, out["t"].ctypes.data,
                                               out["obj"].ctypes.data, out["normal"].ctypes.data,
                                               out["position"].ctypes.data, out["uv"].ctypes.data,
                                               out["bary"].ctypes.data, out["basecolor"].ctypes.data),
              "jsrt_material_data")
        return out

    def material_uv(self, rays):
        """The UV pair the base material's colour chains read at each ray's closest hit, after any
        PositionalUVMaterial above the material (include/jsrt.h jsrt_material_uv): (uv n x 2 f32, has_uv n i32);
        has_uv 0 = a miss, or a hit whose material_data has no UV (the pair is NaN)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = len(rays)
        uv = np.empty((n, 2), np.float32)
        has = np.empty(n, np.int32)
        check(_native.posuv_api().jsrt_material_uv(self._h, rays.ctypes.data, n, uv.ctypes.data, has.ctypes.data),
              "jsrt_material_uv")
        return uv, has

    def sdf_distance(self, obj, points):
        """SDF.distance of SDFGeometry primitive `obj` (OBJS index) at local points (include/jsrt.h)."""
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        out = np.empty(len(points), np.float64)
        check(_native.lib().jsrt_sdf_distance(self._h, int(obj), points.ctypes.data, len(points), out.ctypes.data),
              "jsrt_sdf_distance")
        return out

    def sdf_forms(self):
        """What the loader decided for this scene's SDFGeometry primitives (include/jsrt.h jsrt_scene_sdf_forms):
        {"all_forms": 0 / 1, "roots": {OBJS index: form id of its root's program, 0 = the program VM}}."""
        return _sdf_forms(lambda *a: _native.lib().jsrt_scene_sdf_forms(self._h, *a), "jsrt_scene_sdf_forms")

    def material_color(self, mcolor, uv):
        """MaterialColor.color({UV}) of MCOL record `mcolor` (a solid, scaled, checkerboard or texture chain) at
        uv (n x 2 f32) on the device (include/jsrt.h jsrt_material_color): n x 3 f32, r g b."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        out = np.empty((len(uv), 3), np.float32)
        check(_native.texture_api().jsrt_material_color(self._h, int(mcolor), uv.ctypes.data, len(uv), out.ctypes.data),
              "jsrt_material_color")
        return out

    def color(self, rays, keys=None, *, max_depth=None, seed=1, sample0=0, spp=1, max_paths=0, stats=None):
        """World.color (world.js:31-41) of caller-supplied rays (include/jsrt_color.h): rays n x 6 f32 (origin xyz
        w=1, direction xyz w=0), keys n u32 (None: the ray's index); sample s of ray i draws from the keyed generator
        at (seed, pixel = keys[i], sample = sample0 + s).  max_depth None: the blob's maxRecursionDepth; 0: black.
        numpy in: (n, spp, 3) float32 out, through the host.  A torch tensor on the scene's device in: jsrt_color_device
        on the current torch stream, a device tensor out, no host copy.  stats: a dict that receives the call's stats."""
        L = _native.color_api()
        spp = max(1, int(spp))
        cp = _native.ColorParams(-1 if max_depth is None else int(max_depth), int(seed) & 0xFFFFFFFF, int(sample0), spp,
                                 int(max_paths))
        st = Stats() if stats is not None else None
        st_ref = ctypes.byref(st) if st is not None else None
        if isinstance(rays, np.ndarray) or not hasattr(rays, "data_ptr"):
            rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
            n = len(rays)
            if keys is not None:
                keys = np.ascontiguousarray(keys, np.uint32).reshape(-1)
                if len(keys) != n:
                    raise JsrtError("keys must hold one key per ray")
            out = np.empty((n, spp, 3), np.float32)
            check(L.jsrt_color(self._h, rays.ctypes.data, keys.ctypes.data if keys is not None else None, n,
                               ctypes.byref(cp), out.ctypes.data, st_ref), "jsrt_color")
        else:
            import torch
            if not rays.is_cuda or rays.device.index != self.device:
                raise JsrtError(f"rays must be on the scene's device (cuda:{self.device})")
            rays = rays.to(torch.float32).contiguous().reshape(-1, 6)
            n = rays.shape[0]
            kt = None
            if keys is not None:
                if not hasattr(keys, "data_ptr"):
                    keys = torch.as_tensor(np.ascontiguousarray(keys, np.uint32).view(np.int32), device=rays.device)
                if keys.device != rays.device or keys.element_size() != 4 or keys.numel() != n:
                    raise JsrtError("keys must be n 32-bit integers on the rays' device")
                kt = keys.contiguous()
            out = torch.empty((n, spp, 3), dtype=torch.float32, device=rays.device)
            with torch.cuda.device(rays.device):
                stream = torch.cuda.current_stream().cuda_stream
                check(L.jsrt_color_device(self._h, rays.data_ptr() if n else None, kt.data_ptr() if kt is not None and n else None,
                                          n, ctypes.byref(cp), out.data_ptr() if n else None, stream, st_ref),
                      "jsrt_color_device")
        if st is not None:
            stats.update(st.as_dict())
        return out

    def camera_rays(self, width=0, height=0, kind=-1, seed=1, sample=0):
        """The rays a render of width x height with renderer `kind` and `seed` starts for sample index `sample`
        (include/jsrt_color.h jsrt_camera_rays; Camera.getRayForPixel with the sampling renderers' jitter and the
        camera's depth-of-field draws): (H * W, 6) float32 in pixel order py * W + px."""
        L = _native.color_api()
        hdr = self.header()
        W = width if width > 0 else hdr["width"]
        H = height if height > 0 else hdr["height"]
        p = self.params(W, H, kind=kind, seed=seed, device=self.device)
        out = np.empty((H * W, 6), np.float32)
        check(L.jsrt_camera_rays(self._h, ctypes.byref(p), int(sample), out.ctypes.data), "jsrt_camera_rays")
        return out

    def camera(self):
        """The Camera the scene's blob was loaded with (include/jsrt_views.h jsrt_scene_camera)."""
        r = _native.CameraRec()
        check(_native.views_api().jsrt_scene_camera(self._h, ctypes.byref(r)), "jsrt_scene_camera")
        return Camera._from_rec(r)

    def render_views(self, cameras, width=0, height=0, spp=0, max_depth=0, kind=-1, seed=1, view_seeds=None, max_paths=0,
                     want_colors=False, device=False, stats=None, stage_events=0, mode=None, **params):
        """One frame per Camera of `cameras`, all in one wavefront batch (include/jsrt_views.h): view v is, bit for
        bit, Scene(with_camera(blob, cameras[v])).render(...) with the same arguments and the seed view_seeds[v]
        (None: `seed` for every view).  Returns rgba uint8 (V, H, W, 4), or (rgba, colors float32 (V, H, W, 4)) with
        want_colors.  device=True: torch tensors on the scene's device, rendered on the current torch stream through
        jsrt_render_views_device, no host copy.  stats: a dict that receives the call's stats.  Further keyword
        arguments are jsrt_params fields (the library refuses x_offset, x_delt > 1 and a foreign device_mask)."""
        L = _native.views_api()
        cameras = list(cameras)
        nv = len(cameras)
        recs = (_native.CameraRec * max(nv, 1))(*[c._rec() for c in cameras])
        seeds = None
        if view_seeds is not None:
            seeds = np.ascontiguousarray(view_seeds, np.uint32).reshape(-1)
            if len(seeds) != nv:
                raise JsrtError("view_seeds must hold one seed per camera")
        p = self.params(width, height, spp, max_depth, kind, int(seed) & 0xFFFFFFFF, device=self.device, max_paths=max_paths,
                        stage_events=stage_events, mode=mode_code(mode), **params)
        hdr = self.header()
        W = width if width > 0 else hdr["width"]
        H = height if height > 0 else hdr["height"]
        st = Stats() if stats is not None else None
        st_ref = ctypes.byref(st) if st is not None else None
        seeds_ptr = seeds.ctypes.data if seeds is not None else None
        shape = (max(nv, 0), H, W, 4)
        if not device:
            rgba = np.zeros(shape, np.uint8)
            colors = np.full(shape, np.nan, np.float32) if want_colors else None
            check(L.jsrt_render_views(self._h, ctypes.byref(p), recs, nv, seeds_ptr, rgba.ctypes.data,
                                      colors.ctypes.data if colors is not None else None, st_ref), "jsrt_render_views")
        else:
            import torch
            dev = torch.device("cuda", self.device)
            rgba = torch.zeros(shape, dtype=torch.uint8, device=dev)
            colors = torch.full(shape, float("nan"), dtype=torch.float32, device=dev) if want_colors else None
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream().cuda_stream
                check(L.jsrt_render_views_device(self._h, ctypes.byref(p), recs, nv, seeds_ptr, rgba.data_ptr(),
                                                 colors.data_ptr() if colors is not None else None, stream, st_ref),
                      "jsrt_render_views_device")
        if st is not None:
            stats.update(st.as_dict())
        return (rgba, colors) if want_colors else rgba

    def close(self):
        if getattr(self, "_h", None):
            _native.lib().jsrt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def params(width=0, height=0, spp=0, max_depth=0, kind=-1, seed=1, x_offset=0, x_delt=1, device=0,
               samples_per_launch=0, timelimit_ms=0.0, max_paths=0, stage_events=0, mode=MODE_STRICT, device_mask=0):
        return Params(width, height, spp, max_depth, kind, seed, x_offset, x_delt, device, samples_per_launch,
                      timelimit_ms, max_paths, stage_events, mode, device_mask)

    def render(self, width=0, height=0, spp=0, max_depth=0, kind=-1, seed=1, x_offset=0, x_delt=1,
               samples_per_launch=0, rgba=None, want_colors=True, progress=None, timelimit_ms=0.0, max_paths=0,
               mode=None, device_mask=0):
        """Render into host arrays.  Returns (rgba u8[H,W,4], colors f32[H,W,4] or None, stats).
        mode: "strict" (the only numeric mode built; "fast" raises) or MODE_*; device_mask: bit d = HIP device d
        renders part of the columns (jsrt.h jsrt_params::device_mask; 0 = the scene's device)."""
        L = _native.lib()
        p = self.params(width, height, spp, max_depth, kind, seed, x_offset, x_delt, self.device,
                        samples_per_launch, timelimit_ms, max_paths, mode=mode_code(mode), device_mask=device_mask)
        W = width if width > 0 else self.header()["width"]
        H = height if height > 0 else self.header()["height"]
        if rgba is None:
            rgba = np.zeros((H, W, 4), np.uint8)
        assert rgba.shape == (H, W, 4) and rgba.dtype == np.uint8 and rgba.flags.c_contiguous
        colors = np.full((H, W, 4), np.nan, np.float32) if want_colors else None
        st = Stats()
        cb = PROGRESS_NONE
        if progress is not None:
            cb = _native.PROGRESS_FN(lambda ps, c, u: progress(int(ps), float(c)))
        rc = L.jsrt_render(self._h, ctypes.byref(p), rgba.ctypes.data,
                           colors.ctypes.data if colors is not None else None, cb, None, ctypes.byref(st))
        check(rc, "jsrt_render")
        return rgba, colors, st.as_dict()

    def render_device(self, d_rgba_ptr, d_colors_ptr=None, stream_ptr=0, col_block=1, stats=True, progress=None,
                      progress_ex=None, **kw):
        """Render owned columns into device buffers (see jsrt.h jsrt_render_device).  stats=False
        records no per-launch HIP events (and returns None).  progress(pass, completion): called at the
        timelimit_ms cadence with the device buffers holding the running mean of the passes done (Incremental;
        jsrt_render_device_progress) -- synchronous, the stream idle in the callback.
        progress_ex(pass, completion, clean) -> truthy to abort (jsrt_render_device_progress_ex): called for every
        reported pass, clean or not (the multi-rank form, tiles.render_progressive); an exception it raises
        aborts the frame and is re-raised here."""
        L = _native.lib()
        p = self.params(device=self.device, **kw)
        st = Stats() if stats else None
        if progress is None and progress_ex is None:
            rc = L.jsrt_render_device(self._h, ctypes.byref(p), col_block, d_rgba_ptr, d_colors_ptr, stream_ptr,
                                      ctypes.byref(st) if stats else None)
            check(rc, "jsrt_render_device")
            return st.as_dict() if stats else None
        err = []
        if progress_ex is not None:
            def tramp_ex(pass_, completion, clean, _user):
                try:
                    return 1 if progress_ex(int(pass_), float(completion), bool(clean)) else 0
                except BaseException as e:  # noqa: BLE001 -- re-raised after the frame
                    err.append(e)
                    return 1
            cb = _native.PROGRESS_EX_FN(tramp_ex)
            rc = L.jsrt_render_device_progress_ex(self._h, ctypes.byref(p), col_block, d_rgba_ptr, d_colors_ptr,
                                                  stream_ptr, cb, None, ctypes.byref(st) if stats else None)
            if err:
                raise err[0]
            if rc == _native.RC_ABORTED:
                return None
            check(rc, "jsrt_render_device_progress_ex")
            return st.as_dict() if stats else None

        def tramp(pass_, completion, _user):
            try:
                progress(int(pass_), float(completion))
            except BaseException as e:  # noqa: BLE001 -- re-raised after the frame
                err.append(e)
        cb = _native.PROGRESS_FN(tramp)
        rc = L.jsrt_render_device_progress(self._h, ctypes.byref(p), col_block, d_rgba_ptr, d_colors_ptr, stream_ptr,
                                           cb, None, ctypes.byref(st) if stats else None)
        if err:
            raise err[0]
        check(rc, "jsrt_render_device_progress")
        return st.as_dict() if stats else None

    def render_device_accum(self, d_accum_ptr, stream_ptr=0, col_block=1, stats=True, **kw):
        """Render owned columns into a device f32 accumulator (jsrt.h jsrt_render_device_accum: ncols * H * 4 f32,
        [owned column][row], w = 0), the multi-GPU accumulator exchange's tile; no RGBA8."""
        L = _native.lib()
        p = self.params(device=self.device, **kw)
        st = Stats() if stats else None
        check(L.jsrt_render_device_accum(self._h, ctypes.byref(p), col_block, d_accum_ptr, stream_ptr,
                                         ctypes.byref(st) if stats else None), "jsrt_render_device_accum")
        return st.as_dict() if stats else None

    def header(self):
        return scene_header(self._blob)


PROGRESS_NONE = ctypes.cast(None, _native.PROGRESS_FN)


def finish_accum(d_accum_ptr, n, kind, passes, d_rgba_ptr, d_colors_ptr=None, stream_ptr=0):
    """setColor of n device accumulators (jsrt.h jsrt_finish_accum): RGBA8 (+ f32 colours) on a device stream."""
    check(_native.lib().jsrt_finish_accum(d_accum_ptr, int(n), int(kind), int(passes), d_rgba_ptr, d_colors_ptr,
                                          stream_ptr), "jsrt_finish_accum")


def owned_columns(width, x_offset, x_delt, col_block=1):
    return int(_native.lib().jsrt_owned_columns(width, x_offset, x_delt, col_block))


def _sdf_forms(call, what):
    allf, count = ctypes.c_int32(), ctypes.c_size_t()
    check(call(ctypes.byref(allf), None, None, 0, ctypes.byref(count)), what)
    n = count.value
    objs, forms = (ctypes.c_int32 * max(n, 1))(), (ctypes.c_int32 * max(n, 1))()
    check(call(ctypes.byref(allf), objs, forms, n, ctypes.byref(count)), what)
    return {"all_forms": int(allf.value), "roots": {int(objs[i]): int(forms[i]) for i in range(n)}}


def sdf_forms(blob):
    """Scene.sdf_forms of a blob without a GPU (include/jsrt.h jsrt_sdf_forms): the loader runs on the host, and
    raises JsrtError for a scene it refuses, as Scene(blob) would."""
    blob = bytes(blob)
    buf = ctypes.create_string_buffer(blob, len(blob))
    return _sdf_forms(lambda *a: _native.lib().jsrt_sdf_forms(buf, len(blob), *a), "jsrt_sdf_forms")


def scene_header(blob):
    import struct
    magic, version, nsec, _ = struct.unpack_from("<4I", blob, 0)
    if magic != 0x5452534A or version != 1:
        raise JsrtError("not a JSRT v1 scene blob")
    for i in range(nsec):
        tag, count, off, nbytes = struct.unpack_from("<IIQQ", blob, 16 + 24 * i)
        if tag == 0x52444E52:  # 'RNDR'
            kind, spp, depth, w, h = struct.unpack_from("<5I", blob, off)
            return {"kind": kind, "spp": spp, "max_depth": depth, "width": w, "height": h}
    raise JsrtError("scene blob has no renderer record")


TEXTURE_MODES = {"bilinear": 0, "nearest": 1}  # include/jsrt_scene.h JSRT_TEX_*


def set_texture(blob, mcolor, image, mode="bilinear", clampU=True, clampV=True):
    """A copy of `blob` in which MCOL record `mcolor` is TextureMaterialColor(image, mode, clampU, clampV)
    (materials.js:78-87; include/jsrt_texture.h jsrt_blob_set_texture): the way to texture a scene that came from
    JSON or OBJ ingest.  image: (H, W, 4) uint8, ImageData order (RGBA, top row first).  Host-only; whether the
    slots the record sits in accept a texture is decided by Scene(...)."""
    if mode not in TEXTURE_MODES:
        raise JsrtError(f"unsupported texture mode {mode!r}")
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 4:
        raise JsrtError("image must be an (H, W, 4) uint8 array")
    image = np.ascontiguousarray(image)
    blob = bytes(blob)
    L = _native.texture_api()
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    check(L.jsrt_blob_set_texture(blob, len(blob), int(mcolor), image.ctypes.data, image.shape[1], image.shape[0],
                                  TEXTURE_MODES[mode], int(bool(clampU)), int(bool(clampV)), ctypes.byref(out),
                                  ctypes.byref(n)), "jsrt_blob_set_texture")
    try:
        return ctypes.string_at(out, n.value)
    finally:
        L.jsrt_blob_free(out)


class HipRenderer:
    """Drop-in for SimpleRenderer / IncrementalMultisamplingRenderer / RandomMultisamplingRenderer
    (renderers.js).  ``scene`` is a Scene (or blob); kind/spp/depth default to the blob's renderer."""

    def __init__(self, scene, samplesPerPixel=None, maxRecursionDepth=None, kind=None, seed=1, device=0, mode="strict",
                 device_mask=0):
        self.scene = scene if isinstance(scene, Scene) else Scene(scene, device)
        self.mode, self.device_mask = mode, device_mask  # jsrt_params::mode / device_mask
        hdr = self.scene.header()
        self.kind = hdr["kind"] if kind is None else (RENDERER_KINDS[kind] if isinstance(kind, str) else kind)
        self.samplesPerPixel = hdr["spp"] if samplesPerPixel is None else samplesPerPixel
        self.maxRecursionDepth = hdr["max_depth"] if maxRecursionDepth is None else maxRecursionDepth
        self.seed = seed

    @staticmethod
    def computePixelCount(img, x_offset, x_delt):  # renderers.js:7-9
        return ((img.width() / x_delt) + round(1 - x_offset / x_delt) * (img.width() % x_delt)) * img.height()

    def render(self, img, timelimit=0, callback=False, x_offset=0, x_delt=1):
        if x_delt <= 0:
            raise JsrtError("x_delt must be positive")
        progress = None
        spl = 0
        if timelimit and callback:
            # the Incremental renderer reports per pass (renderers.js:103-112): one sample per pixel per
            # launch, so each callback sees that pass's running mean in img; other kinds report on the
            # library's batches
            spl = 1 if self.kind == RENDERER_KINDS["IncrementalMultisamplingRenderer"] else 0

            def progress(p, c):
                callback({"pass": p, "completion": c})
        self.scene.render(img.width(), img.height(), self.samplesPerPixel, self.maxRecursionDepth, self.kind,
                          self.seed, x_offset, x_delt, samples_per_launch=spl, rgba=img.imgdata, want_colors=False,
                          progress=progress, timelimit_ms=float(timelimit or 0), mode=self.mode,
                          device_mask=self.device_mask)
        return img
