// jsrt_node_color.cpp — Node N-API addon over include/jsrt_color.h: World.color of caller-supplied rays.
//
// A module of its own (jsrt_node_color.node) beside jsrt_node.node, whose scene handles it takes:
//
//   color(scene, rays: Float32Array (n x 6), keys: Uint32Array (n) | null, params) -> Promise<Float32Array>
//       params: {maxRecursionDepth (absent / < 0: the blob's), seed = 1, sample0 = 0, samplesPerRay = 1, maxPaths = 0}
//       n x samplesPerRay x 3 f32.  Runs jsrt_color in napi_create_async_work, like jsrt_node.node's render; the
//       inputs and the output stay referenced until it completes, and the scene is kept from sceneDestroy meanwhile.
//
// Errors: argument errors throw; a negative jsrt_color return rejects the promise with jsrt_last_error().
#define NAPI_VERSION 8
#include <node_api.h>
#include <string.h>

#include <string>

#include "../../include/jsrt_color.h"
#include "jsrt_node_scene.h"

namespace {

#define NAPI_OK(call)                                                                   \
    do {                                                                                \
        if ((call) != napi_ok) {                                                        \
            const napi_extended_error_info *ei = nullptr;                               \
            napi_get_last_error_info(env, &ei);                                         \
            napi_throw_error(env, "JSRT_NAPI", ei && ei->error_message ? ei->error_message : #call); \
            return nullptr;                                                             \
        }                                                                               \
    } while (0)

double prop_f64(napi_env env, napi_value obj, const char *name, double dflt) {
    bool has = false;
    napi_has_named_property(env, obj, name, &has);
    if (!has) return dflt;
    napi_value v;
    double r = dflt;
    if (napi_get_named_property(env, obj, name, &v) == napi_ok) napi_get_value_double(env, v, &r);
    return r;
}

// a typed array of the given element type: its data and element count
bool get_typed(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *n) {
    bool is_ta = false;
    napi_is_typedarray(env, v, &is_ta);
    if (!is_ta) return false;
    napi_typedarray_type t;
    napi_value ab;
    size_t off = 0;
    return napi_get_typedarray_info(env, v, &t, n, data, &ab, &off) == napi_ok && t == want;
}

struct ColorJob {
    napi_async_work work = nullptr;
    napi_deferred deferred = nullptr;
    napi_ref rays_ref = nullptr, keys_ref = nullptr, out_ref = nullptr;  // alive while the worker reads / writes them
    napi_ref scene_ref = nullptr;  // keeps the scene external (and its GC finalizer) alive meanwhile
    SceneBox *box = nullptr;
    jsrt_scene *scene = nullptr;
    jsrt_color_params p;
    const float *rays = nullptr;
    const uint32_t *keys = nullptr;
    float *out = nullptr;
    size_t n = 0;
    int rc = 0;
    std::string err;
};

void color_execute(napi_env, void *data) {
    ColorJob *j = static_cast<ColorJob *>(data);
    j->rc = jsrt_color(j->scene, j->rays, j->keys, j->n, &j->p, j->out, nullptr);
    if (j->rc != 0) j->err = jsrt_last_error();  // thread-local: capture on this thread
}

void color_complete(napi_env env, napi_status, void *data) {
    ColorJob *j = static_cast<ColorJob *>(data);
    if (j->rc == 0) {
        napi_value out;
        napi_get_reference_value(env, j->out_ref, &out);
        napi_resolve_deferred(env, j->deferred, out);
    } else {
        napi_value msg, err;
        const std::string m = "jsrt_color: " + j->err;
        napi_create_string_utf8(env, m.c_str(), m.size(), &msg);
        napi_create_error(env, nullptr, msg, &err);
        napi_reject_deferred(env, j->deferred, err);
    }
    for (napi_ref r : {j->rays_ref, j->keys_ref, j->out_ref})
        if (r) napi_delete_reference(env, r);
    scene_job_done(j->box);  // (carries out a sceneDestroy called while this job ran)
    if (j->scene_ref) napi_delete_reference(env, j->scene_ref);
    napi_delete_async_work(env, j->work);
    delete j;
}

napi_value Color(napi_env env, napi_callback_info info) {
    size_t argc = 4;
    napi_value argv[4];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    SceneBox *b = argc > 0 ? get_scene(env, argv[0]) : nullptr;
    if (!b || !b->s || b->destroy_pending) {
        napi_throw_type_error(env, "JSRT", "color: scene handle is missing or destroyed");
        return nullptr;
    }
    void *rays = nullptr, *keys = nullptr;
    size_t nr = 0, nk = 0;
    if (argc < 2 || !get_typed(env, argv[1], napi_float32_array, &rays, &nr) || nr % 6 != 0) {
        napi_throw_type_error(env, "JSRT", "color: rays must be a Float32Array of n * 6 (origin xyz, direction xyz)");
        return nullptr;
    }
    const size_t n = nr / 6;
    napi_valuetype kt = napi_undefined;
    if (argc > 2) napi_typeof(env, argv[2], &kt);
    const bool have_keys = kt != napi_undefined && kt != napi_null;
    if (have_keys && (!get_typed(env, argv[2], napi_uint32_array, &keys, &nk) || nk != n)) {
        napi_throw_type_error(env, "JSRT", "color: keys must be a Uint32Array of one key per ray, or null");
        return nullptr;
    }
    jsrt_color_params p;
    memset(&p, 0, sizeof p);
    p.max_depth = -1;
    p.seed = 1;
    p.spp = 1;
    napi_valuetype pt = napi_undefined;
    if (argc > 3) napi_typeof(env, argv[3], &pt);
    if (pt == napi_object) {
        p.max_depth = (int32_t)prop_f64(env, argv[3], "maxRecursionDepth", -1);
        p.seed = (uint32_t)prop_f64(env, argv[3], "seed", 1);
        p.sample0 = (uint32_t)prop_f64(env, argv[3], "sample0", 0);
        p.spp = (int32_t)prop_f64(env, argv[3], "samplesPerRay", 1);
        p.max_paths = (int32_t)prop_f64(env, argv[3], "maxPaths", 0);
    }
    if (p.spp <= 0) p.spp = 1;
    if ((double)n * (double)p.spp > 2147483648.0) {  // (also before the output is allocated)
        napi_throw_range_error(env, "JSRT", "color: n * samplesPerRay above 2^31 paths is not supported");
        return nullptr;
    }
    const size_t nout = n * (size_t)p.spp * 3;
    napi_value ab, out;
    void *outp = nullptr;
    NAPI_OK(napi_create_arraybuffer(env, nout * sizeof(float), &outp, &ab));
    NAPI_OK(napi_create_typedarray(env, napi_float32_array, nout, ab, 0, &out));
    ColorJob *j = new ColorJob();
    j->scene = b->s;
    j->p = p;
    j->rays = static_cast<const float *>(rays);
    j->keys = have_keys ? static_cast<const uint32_t *>(keys) : nullptr;
    j->out = static_cast<float *>(outp);
    j->n = n;
    napi_value promise, name;
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok) {
        delete j;
        napi_throw_error(env, "JSRT_NAPI", "color: napi_create_promise failed");
        return nullptr;
    }
    napi_create_reference(env, argv[1], 1, &j->rays_ref);
    if (have_keys) napi_create_reference(env, argv[2], 1, &j->keys_ref);
    napi_create_reference(env, out, 1, &j->out_ref);
    napi_create_reference(env, argv[0], 1, &j->scene_ref);
    j->box = b;
    ++b->inflight;
    napi_create_string_utf8(env, "jsrt_color", NAPI_AUTO_LENGTH, &name);
    if (napi_create_async_work(env, nullptr, name, color_execute, color_complete, j, &j->work) != napi_ok ||
        napi_queue_async_work(env, j->work) != napi_ok) {
        j->rc = -3;
        j->err = "the async work could not be queued";
        if (!j->work) {  // nothing to delete: complete by hand
            napi_value msg, err;
            napi_create_string_utf8(env, j->err.c_str(), j->err.size(), &msg);
            napi_create_error(env, nullptr, msg, &err);
            napi_reject_deferred(env, j->deferred, err);
            for (napi_ref r : {j->rays_ref, j->keys_ref, j->out_ref, j->scene_ref})
                if (r) napi_delete_reference(env, r);
            scene_job_done(j->box);
            delete j;
        } else {
            color_complete(env, napi_generic_failure, j);
        }
    }
    return promise;
}

napi_value Init(napi_env env, napi_value exports) {
    const napi_property_descriptor props[] = {
        {"color", nullptr, Color, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
    };
    napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
