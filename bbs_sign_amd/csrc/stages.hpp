// Per-item device stages of the four batched BBS+ core operations.
//
// Every stage is a __host__ __device__ "item function" run by one GPU lane; the __global__
// wrappers live in capi.hip.  Batch data is SoA in HBM: word w of item i of an array is at
// base[w * n + i], so the 64 lanes of a wavefront (64 consecutive items) read 256 contiguous
// bytes per word -- coalesced.
//
// Work split (MI355X: 1024 SIMDs, a batch of 4096 items is only 64 wavefronts, so each item is
// split over several lanes wherever the algebra allows):
//   * a multi-scalar multiplication is cut into PARTS -- a variable-base scalar multiplication (or the
//     joint multiplication of T1's three terms), plus NFIX chunks of the fixed-base (windowed,
//     precomputed-table) sum -- every part on its own lane (part-major thread index: a wavefront runs
//     one kind of part);
//   * a pairing product is sliced over six lanes per item (pairing_dist.hpp, stage PairDist); the
//     one-lane PairMiller / PairFinal stages below serve the CPU-side test build only.
//
// Algebraic restructurings (bit-identical group elements / booleans):
//   proof_verify: T2 = Bv*c + D*r3^ + sum H_j m^_j  with  Bv = P1 + Q1*domain + sum H_i m_i
//                 (src/proof_verify.rs:165-182) is evaluated as ONE fixed-base sum over
//                 {P1, Q1, H_*} with scalars {c, domain*c, m_i*c | m^_j} plus D*r3^.
//   verify      : e(A, W + e*BP2) * e(B, -BP2) == 1  (src/verify.rs:88-92)
//                 <=>  e(A, W) * e(e*A - B, BP2) == 1 : both G2 arguments fixed.
//   sign        : A = B * (sk+e)^-1 (src/sign.rs:128-130) = fixed-base sum with scalars * inv.
//   proof_gen   : D, Abar, Bbar, T1, T2 (src/proof_gen.rs:249-263) as fixed-base sums over B's
//                 terms plus scalar multiples of the signature point A.
#pragma once
#include "stages_common.hpp"
#include "stages_pair.hpp"
#include "stages_pv.hpp"
#include "stages_vf.hpp"
#include "stages_sg.hpp"
#include "stages_pg.hpp"
#include "stages_draw.hpp"
#include "stages_prim.hpp"
