// kernels_trr.h — k_trr_unpack: big-endian f32 / f64 positions of GROMACS TRR frames -> f32 coordinates of the analysed
// atoms, on the device.  Part of the single translation unit gorder_hip.hip; device code for gfx950 only.
//
// What it replaces: the conversion loop of the host's TRR reader (trr_next in xtc_reader.cpp; the reference reads TRR
// through groan_rs' TrrReader, common.rs:306-320).  There is nothing to decompress: the host copies the leading
// n_stop * 3 reals of every selected frame's positions block (gorder_xtc_pack_window on a TRR reader; bits 2 / 3 of
// gorder_xtc_frame_t::kind say f32 / f64) and this kernel swaps the bytes and, for doubles, rounds to f32 the way the
// host's `(float)` cast does — same floats as gorder_xtc_next, bit for bit (tests/test_trr_device_gpu.py).
//
// A pure stream: 12 bytes in + 12 bytes out per analysed atom for f32 files, 24 + 12 for f64.  No LDS, no atomics
// (but the error word), plain vector loads and stores.
#pragma once

#include "../../include/gorder_xtc.h"
#include "trr_round.h"

namespace {

constexpr uint32_t kTrrKindF32 = 4u, kTrrKindF64 = 8u;     // bits 2 and 3 of gorder_xtc_frame_t::kind
constexpr uint32_t kTrrBlock = 256;

// 16 bytes at an address that is only a multiple of 4 (one global_load_dwordx4: vector memory needs dword alignment)
typedef uint32_t trr_u32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) TrrQuadA4 { trr_u32x4 v; };
struct __attribute__((aligned(16))) TrrQuadA16 { trr_u32x4 v; };

__device__ __forceinline__ trr_u32x4 trr_load16(const uint32_t *p) { return reinterpret_cast<const TrrQuadA4 *>(p)->v; }

// real k of a frame's block (big-endian, `dbl`: 8 bytes) as the bits of the f32
__device__ __forceinline__ uint32_t trr_real(const uint32_t *__restrict__ w, size_t k, bool dbl) {
    if (!dbl) return __builtin_bswap32(w[k]);
    const unsigned long long hi = __builtin_bswap32(w[2u * k]), lo = __builtin_bswap32(w[2u * k + 1u]);
    return trr_f64_bits_to_f32_bits((hi << 32) | lo);
}

// grid = (pieces of a frame, frames — a block takes frames blockIdx.y, blockIdx.y + gridDim.y, ...), 256 threads.
//   blob, frames : what gorder_xtc_pack_window produced from TRR readers (device copies); frames of another kind are
//                  passed over (the XTC kernels decode those)
//   natoms       : atoms per frame in the file;  n_stop: atoms that were copied (up to the last analysed one)
//   slot_of      : [natoms] output slot of an atom or -1; null: atom t goes to slot t, t < n_stop
//   out          : [n_frames][n_out][3]
// Without slot_of a frame is ONE stream of 3 n_stop reals.  A thread makes four consecutive floats of it, from 16 (f32) or
// 32 (f64) consecutive bytes of the block, and writes them with one 16-byte store: the quads are laid out from the first
// 16-byte boundary of the OUTPUT frame (a frame starts at 12 n_out fr bytes: 0, 4, 8 or 12 modulo 16), so the loads are
// the ones that may lie across 16-byte boundaries (they only need dword alignment).  The up to three floats before the
// first boundary and behind the last one are written one by one by the thread behind the last quad.
// With slot_of: a thread per atom, three dword stores into its slot; atoms without a slot are read over.
// Never reads past the block's n_stop * 3 reals (which the zero padding follows), never writes outside the frame.
__global__ __launch_bounds__(kTrrBlock) void k_trr_unpack(const uint8_t *__restrict__ blob, unsigned long long blob_bytes,
                                                         const gorder_xtc_frame_t *__restrict__ frames, uint32_t n_frames,
                                                         uint32_t natoms, const int32_t *__restrict__ slot_of, uint32_t n_stop,
                                                         float *__restrict__ out, uint32_t n_out, uint32_t *err) {
    const unsigned long long tid = (unsigned long long)blockIdx.x * kTrrBlock + threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * kTrrBlock;
    const unsigned long long n_reals = 3ull * n_stop;
    for (uint32_t fr = blockIdx.y; fr < n_frames; fr += gridDim.y) {
        const gorder_xtc_frame_t d = frames[fr];
        if (!(d.kind & (kTrrKindF32 | kTrrKindF64))) continue;                 // an XTC frame of a mixed table
        const bool dbl = (d.kind & kTrrKindF64) != 0u;
        const unsigned long long region = (((unsigned long long)d.n_bytes + 63ull) & ~63ull) + 64ull;
        const bool bad = (d.offset & 63ull) != 0ull || d.offset + region > blob_bytes || d.offset + region < d.offset ||
                         (unsigned long long)d.n_bytes < n_reals * (dbl ? 8ull : 4ull) || n_stop > natoms ||
                         (!slot_of && n_out < n_stop);
        if (bad) {
            if (tid == 0ull) raise_error(err, GORDER_ERR_TRAJECTORY_FORMAT, fr, kStageBox);
            continue;
        }
        const uint32_t *w = reinterpret_cast<const uint32_t *>(blob + d.offset);
        uint32_t *o = reinterpret_cast<uint32_t *>(out) + (size_t)fr * n_out * 3u;
        if (slot_of) {
            for (unsigned long long t = tid; t < n_stop; t += stride) {
                const int32_t slot = slot_of[t];
                if (slot < 0 || (uint32_t)slot >= n_out) continue;
                uint32_t *q = o + 3u * (size_t)slot;
                q[0] = trr_real(w, 3u * (size_t)t, dbl);
                q[1] = trr_real(w, 3u * (size_t)t + 1u, dbl);
                q[2] = trr_real(w, 3u * (size_t)t + 2u, dbl);
            }
            continue;
        }
        // floats before the first 16-byte boundary of the output frame, whole quads, floats behind the last quad
        const unsigned long long head = min((unsigned long long)((4u - (uint32_t)((reinterpret_cast<uintptr_t>(o) >> 2) & 3u)) & 3u), n_reals);
        const unsigned long long n_quads = (n_reals - head) >> 2;
        for (unsigned long long j = tid; j <= n_quads; j += stride) {
            const unsigned long long k = head + 4ull * j;                     // first real of the quad
            if (j == n_quads) {                                                // the thread behind the last quad: head and tail
                for (unsigned long long i = 0; i < head; i++) o[i] = trr_real(w, i, dbl);
                for (unsigned long long i = k; i < n_reals; i++) o[i] = trr_real(w, i, dbl);
                break;
            }
            trr_u32x4 r;
            if (!dbl) {
                const trr_u32x4 a = trr_load16(w + k);
                r.x = __builtin_bswap32(a.x); r.y = __builtin_bswap32(a.y);
                r.z = __builtin_bswap32(a.z); r.w = __builtin_bswap32(a.w);
            } else {
                const trr_u32x4 a = trr_load16(w + 2ull * k), b = trr_load16(w + 2ull * k + 4ull);
                r.x = trr_f64_bits_to_f32_bits(((unsigned long long)__builtin_bswap32(a.x) << 32) | __builtin_bswap32(a.y));
                r.y = trr_f64_bits_to_f32_bits(((unsigned long long)__builtin_bswap32(a.z) << 32) | __builtin_bswap32(a.w));
                r.z = trr_f64_bits_to_f32_bits(((unsigned long long)__builtin_bswap32(b.x) << 32) | __builtin_bswap32(b.y));
                r.w = trr_f64_bits_to_f32_bits(((unsigned long long)__builtin_bswap32(b.z) << 32) | __builtin_bswap32(b.w));
            }
            reinterpret_cast<TrrQuadA16 *>(o + k)->v = r;
        }
    }
}

}  // namespace
