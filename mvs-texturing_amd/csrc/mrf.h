// mrf.h -- what more than one of the MRF solver's three sources needs (k_mrf_setup.hip: the tables, k_mrf_sweep.hip: the sweeps,
// k_mrf_polish.hip: whatever works on a labeling afterwards).  Internal, host-and-device.  Something a single file uses stays in that
// file; the prototypes other files call are ctx.h's.
#pragma once
#include "ctx.h"

namespace mvs {

constexpr uint16_t MAP_NONE = 0xFFFF;   // a 16-bit map entry of a generic sender: the label is absent from its list

// Messages live in HBM as 8-bit fixed point over their range [0, lam], lam = 1 / rho (a message is a truncated,
// min-normalised cavity: 0 <= m <= lam by construction); arithmetic is fp32.  code = trunc(m * (255 / lam) + 0.5),
// value = code * (lam / 255): a quarter of the bytes of an fp32 layout, half of binary16, at the same solution
// quality (part of the solver's definition, restated in oracle/oracle.cpp).
typedef uint8_t msg_t;

// Schedule order = nodes sorted by SUB-CLASS key: fast nodes first, by (colour, class, id) -- key = 4 * colour + class < 256 --
// then the generic nodes by (colour, id) -- key = 256 + colour.  Every (colour, class) pair is one contiguous range of the
// order = one launch; the fast nodes (their records and descriptors) are positions [0, n_fast).
constexpr uint32_t N_SUB = 320;            // sub-classes 0 .. 319 (64 colours x 4 fast classes, 64 generic colour classes)
constexpr uint32_t SUB_GENERIC = 256;
// Every sub-class has two ZONES (sort key = 2 * sub-class + zone): zone 0 = the nodes a sharded caller marked as its BOUNDARY nodes
// (own nodes with an edge into another rank's part: ctx->m_bnd, shard.hip setup_with_marks), zone 1 = everybody else.  A sharded rank sweeps the
// boundary zone of a colour first, hands its runs to the neighbours, and sweeps the interior while they travel; a colour class is an
// independent set, so the split changes no value.  Without marks (single context, building blocks) zone 0 is empty and the order is
// the plain (colour, class, id) order.
constexpr uint32_t N_KEY = 2 * N_SUB;

// The unaries as the sweeps see them: 16-bit fixed point (2 instead of 4 bytes in the records; part of the solver's definition,
// restated in oracle/oracle.cpp)
constexpr float COST_SCALE = 65535.0f;
__device__ __forceinline__ uint32_t cost_code(float c) { return (uint32_t)(c * COST_SCALE + 0.5f); }   // c in [0, 1]
__device__ __forceinline__ float cost_value(uint32_t code) { return (float)code * (1.0f / 65535.0f); }

constexpr uint32_t EPART_BLOCKS = 2048;   // per colour phase: upper bound of the blocks of all its launches together (resident blocks)

}  // namespace mvs
