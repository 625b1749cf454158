#!/bin/bash
# Builds the stand-alone host checker (host_check.cpp beside this file) and runs each binary
# directly: plain, under the thread sanitizer, and under the address + undefined-behaviour
# sanitizers.  No library is preloaded and nothing is loaded into Python; no GPU is needed.
#
#   bash tools/host_check/run.sh [-o DIR] [-b] [plain|tsan|asan ...]
#     -o DIR   where the binaries go (default: a fresh temporary directory)
#     -b       build only
#   CXX names the compiler (default: ROCm's clang++, else clang++, else g++).
set -euo pipefail
cd "$(dirname "$0")/../.."
ROCM=${ROCM_PATH:-/opt/rocm}
OUT=
BUILD_ONLY=0
while getopts "o:b" opt; do
  case $opt in
    o) OUT=$OPTARG ;;
    b) BUILD_ONLY=1 ;;
    *) exit 2 ;;
  esac
done
shift $((OPTIND - 1))
[ $# -gt 0 ] || set -- plain tsan asan
[ -n "$OUT" ] || OUT=$(mktemp -d)
mkdir -p "$OUT"
if [ -z "${CXX:-}" ]; then
  for CXX in "$ROCM/lib/llvm/bin/clang++" clang++ g++; do
    command -v "$CXX" > /dev/null && break
  done
fi
for variant in "$@"; do
  case $variant in
    plain) flags="-O2" ;;
    tsan) flags="-O1 -g -fsanitize=thread" ;;
    asan) flags="-O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer" ;;
    *) echo "unknown build '$variant' (plain, tsan, asan)" >&2; exit 2 ;;
  esac
  # (greedy.hpp includes the HIP runtime's header for a type; nothing of the runtime is linked)
  "$CXX" -std=c++17 $flags -Wall -Wextra -pthread -D__HIP_PLATFORM_AMD__ -I "$ROCM/include" -I include \
    -I annealing_sign_problem_amd/csrc tools/host_check/host_check.cpp tools/asan_host/stub.cpp \
    annealing_sign_problem_amd/csrc/sa_plan.cpp annealing_sign_problem_amd/csrc/greedy.cpp \
    -o "$OUT/host_check_$variant"
  echo "built $OUT/host_check_$variant"
  if [ $BUILD_ONLY = 0 ]; then
    "$OUT/host_check_$variant"
  fi
done
