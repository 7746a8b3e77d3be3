#!/bin/bash
# Build the product library of another git revision next to the current one, for same-box A/B runs with tools/quick_perf.py:
#   tools/ab_build.sh <git-ref> [name]   ->  <pkg>/lib/libcrowdnav_<name>.so   (default name: base)
#   CN_LIB=<pkg>/lib/libcrowdnav_base.so python tools/quick_perf.py base; python tools/quick_perf.py new
# No recipe here: the revision is unpacked and built by its own csrc/build.sh (a revision knows how to build itself).
set -euo pipefail
REF="$1"; NAME="${2:-base}"; cd "$(dirname "$0")/.."; ROOT="$PWD"
PKG="drl-based-mapless-crowd-navigation-with-perceived-risk_amd"
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
git archive "$REF" "$PKG/csrc" include | tar -x -C "$T"
bash "$T/$PKG/csrc/build.sh"
mkdir -p "$ROOT/$PKG/lib"; cp "$T/$PKG/lib/libcrowdnav.so" "$ROOT/$PKG/lib/libcrowdnav_$NAME.so"
ls -la "$ROOT/$PKG/lib/libcrowdnav_$NAME.so"
