#!/bin/bash
# Builds tools/trr_pack_sanitize.cpp with the host reader under AddressSanitizer + UBSan and runs it (CPU only).
# usage: tools/trr_pack_sanitize.sh            -> "single precision ok", "double precision ok", exit status 0
set -euo pipefail
cd "$(dirname "$0")/.."
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
${CXX:-g++} -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Iinclude \
    -o "$out/trr_pack_sanitize" tools/trr_pack_sanitize.cpp gorder_amd/csrc/xtc_reader.cpp -lpthread
"$out/trr_pack_sanitize" "$out"
