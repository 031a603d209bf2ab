// jsrt_node_scene.h — the scene handle the N-API addons share: jsrt_node.node creates it (sceneCreate) and
// jsrt_node_color.node takes it (color).  Both run on the JS thread of one process, where every field is touched.
#pragma once
#include <node_api.h>

#include "../../include/jsrt.h"

struct SceneBox {  // the external's payload: destroy is idempotent (explicit + GC finalizer)
    jsrt_scene *s = nullptr;
    int inflight = 0;              // async renders queued or running (all counted on the JS thread)
    bool destroy_pending = false;  // sceneDestroy while renders were in flight: destroyed by the last
};

inline SceneBox *get_scene(napi_env env, napi_value v) {
    void *p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) return nullptr;
    return static_cast<SceneBox *>(p);
}

// an async job of the scene has completed (JS thread): the last one carries out a pending sceneDestroy
inline void scene_job_done(SceneBox *b) {
    if (b && --b->inflight == 0 && b->destroy_pending && b->s) {
        jsrt_scene_destroy(b->s);
        b->s = nullptr;
    }
}
