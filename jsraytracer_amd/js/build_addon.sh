#!/bin/sh
# Builds the Node N-API addons against libjsrt.so: jsraytracer_amd/_build/jsrt_node.node (scenes, renders, ingest)
# and jsrt_node_color.node (World.color of caller-supplied rays, include/jsrt_color.h, over the same scene handles).
# Plain g++ against /usr/include/node (N-API 8, Node 12); no node-gyp.  libjsrt.so is found next to
# the addons through their RUNPATH ($ORIGIN).
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
OUT="$HERE/../_build"
INC="$HERE/../../include"
[ -f "$OUT/libjsrt.so" ] || { echo "build libjsrt.so first (jsraytracer_amd/build.py)" >&2; exit 1; }
[ -f /usr/include/node/node_api.h ] || { echo "node headers missing: skipping the N-API addon" >&2; exit 0; }
# addon <name> <dependency>...: rebuilt when <name>.cpp or a dependency is newer than the module
addon() {
    name=$1
    shift
    fresh=1
    [ -f "$OUT/$name.node" ] || fresh=0
    for d in "$HERE/$name.cpp" "$HERE/jsrt_node_scene.h" "$@"; do
        [ "$fresh" = 1 ] && [ "$OUT/$name.node" -nt "$d" ] || fresh=0
    done
    [ "$fresh" = 1 ] && return 0
    g++ -O2 -std=c++17 -fPIC -shared -Wall -Wextra -Wno-unused-parameter -Wno-missing-field-initializers \
        -DNODE_GYP_MODULE_NAME="$name" -I/usr/include/node \
        "$HERE/$name.cpp" -o "$OUT/$name.node.tmp" \
        -L"$OUT" -ljsrt -Wl,-rpath,'$ORIGIN'
    mv "$OUT/$name.node.tmp" "$OUT/$name.node"
}
addon jsrt_node "$INC/jsrt.h" "$INC/jsrt_mesh.h"
addon jsrt_node_color "$INC/jsrt.h" "$INC/jsrt_color.h"
