// dma_run.hpp — how the list force pass splits one contiguous run of a region row between the two LDS-DMA forms
// (stage_positions_dma, kernels_force_verlet.hip).  Compiles for the host too (tests/hostcpp/dma_run_check.cpp).
//
// A run = n molecules (8 bytes per coordinate) from global index g0 to LDS slot s0, both plain prefix sums of the cell counts (the
// list entries' encoding: no pad slots).  The 16-byte form writes wave-uniform LDS base + lane * 16, so its LDS side must start on an
// EVEN slot; its global side is per lane and may start on any molecule (8-byte aligned dwordx4 sources: checked bit for bit by
// tools/probes/glds_probe.hip).  Hence: an odd first slot goes dword-wise (head), then pairs of slots with the 16-byte form (body),
// then an odd last molecule dword-wise (tail).  Every part lies inside [s0, s0 + n): no instruction touches a slot of another run.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LS1_DMA_HD __host__ __device__
#else
#define LS1_DMA_HD
#endif

namespace ls1 {

struct DmaRunSplit {
	uint32_t head;   // 0 | 1 molecule at slot s0, dword form
	uint32_t pairs;  // 16-byte pieces (two molecules each) from slot s0 + head, an even slot
	uint32_t tail;   // 0 | 1 molecule at slot s0 + head + 2 * pairs, dword form
};

LS1_DMA_HD inline DmaRunSplit dma_run_split(uint32_t s0, uint32_t n) {
	DmaRunSplit r;
	r.head = (n != 0u && (s0 & 1u)) ? 1u : 0u;
	const uint32_t rest = n - r.head;
	r.pairs = rest >> 1;
	r.tail = rest & 1u;
	return r;
}

// wave instructions per coordinate array of a run (64 lanes: 64 pairs per 16-byte instruction, one instruction per dword-wise molecule)
LS1_DMA_HD inline uint32_t dma_run_instructions(const DmaRunSplit& r) { return r.head + (r.pairs + 63u) / 64u + r.tail; }

}  // namespace ls1
