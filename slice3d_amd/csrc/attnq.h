// attnq.h — shared pieces of the query-major attention kernels (decode_attnq.hip: inference / training forward;
// train_attnq.hip: fused training backward): weight-image sizes, the hand-issued ds_read_b32 and the weight ring's barrier
// (the split-precision operand helpers, lane-swap reductions and LDS fragment reads are f16x3.h's).  See decode_attnq.hip
// for the layout story.
#pragma once
#include "decode.h"
#include "dropout.h"

#define AQ_WIN_HALFS (24 * 1024)   // per head: 24 fragment pairs (q0,q1,k0,k1,v0,v1) x 4 k-steps, hi|lo = 48 KiB
#define AQ_WO_HALFS (8 * 1024)     // per head: 8 fragment pairs = 16 KiB

// ---------------------------------------------------------------------------------------------
// Four waves per workgroup, TWO workgroups per CU (one computes while the other sits at a barrier); a workgroup owns
// half a group (8 queries), a wave two of them.  The rows of the wave's two queries are loaded and split ONCE per
// item and stay in registers as f16 hi / lo fragments for the four heads (round 3: the high halves used to be parked in a
// wave-private LDS region and re-read with every k-step — 2 of 6 fragment reads).  The weight ring holds QUARTER-head
// slots of 16 KiB (q | k | v | out_proj fragments), FOUR of them, filled by LDS-DMA three phases ahead; four barriers per
// head; LDS = 4 x 16 KiB ring + 3 KiB of small vectors.
// (Earlier versions: eight waves / whole-head slots / rows re-read per head: 1.16 ms per layer; four waves / half-head
// slots: 1.13 ms; quarter-head slots, two-slot ring: 0.94 ms.  Bench stage, 4 launches + the last layer: 7.41 ms with the
// two-slot ring, 6.9 with full-line stores, 6.86 with the rows in registers, 6.74 with the four-slot ring.)
// ---------------------------------------------------------------------------------------------
// LDS reads and their counted waits are issued by hand (S3D_DS_READ, same finding as in decode_f16.hip's pipelined FFN): with an
// LDS-DMA refill in flight hipcc turns every LDS wait of this single-LDS-object kernel into lgkmcnt(0), i.e. it waits
// for the fragment reads it has just issued for the NEXT k-step (all 42 waits of the previous build were lgkmcnt(0)).
#define AQ_READ32(dst, addr, off) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off) : "memory")
// Four-slot ring, DMA three phases ahead: at a barrier the slot of the phase that starts must have landed, and at most two
// newer DMA sets (2 x 4 instructions per wave) have been issued since — whatever else is in flight (row loads, stores of
// the previous item) is older or only makes the wait stricter.  vmcnt retires in order.  Raw s_barrier: the kernel has no
// compiler-visible LDS access after its prologue, so nothing needs the fence __syncthreads() carries (which would drain vmcnt).
#define AQ_BARRIER()                                       \
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");       \
    asm volatile("s_barrier" ::: "memory")
// The same barrier with the EXACT number of vector-memory operations a wave has issued after the DMA set it waits for (round
// 4).  vmcnt(8) is always safe — at least the two newer DMA sets are younger — but it also waits for all but eight of whatever
// else was issued since: the previous item's row stores and the next rows' loads at the first barriers of an item (32 - 48
// operations), the per-head stores of the training kernels.  n must not exceed the real count (a larger n lets the barrier
// pass before the set has landed), so the callers use these counts only where every counted operation is issued
// unconditionally (T >= 9: both halves of every full-line store pair have active lanes) and fall back to 8 otherwise.
// The counts are hand-derived from the source and hold only while hipcc emits exactly the counted operations (a dropped or
// merged one would let a slot be read before its DMA lands: silently wrong rows).  -DS3D_AQ_SAFE_BARRIERS builds every
// counted barrier as the always-safe vmcnt(8) form; `make` also builds that variant (libslice3d_hip_safe.so) and
// tests/test_gpu_barriers.py holds the two libraries' outputs bit-identical.
#ifdef S3D_AQ_SAFE_BARRIERS
#define AQ_BARRIER_N(n) AQ_BARRIER()
#else
#define AQ_BARRIER_N(n)                                          \
    asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory");        \
    asm volatile("s_barrier" ::: "memory")
#endif
#define AQ3_SLOT_HALFS (8 * 1024)    // 8 fragment pairs = 16 KiB
