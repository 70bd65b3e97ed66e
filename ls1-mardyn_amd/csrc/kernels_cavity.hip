// kernels_cavity.hip — cavity detection on the device: the neighbour counts of the reference's CavityWriter plugin (io/CavityWriter.cpp:
// 160-174) over the node lattice of its CavityEnsemble (ensemble/CavityEnsemble.cpp:114-219 the lattice, :280-311 countNeighbours,
// :254-259 decideActivity).
//
// The work is split over the NODE LATTICE, not over molecules or cells: the lattice is regular, so a box of nodes shares one set of
// candidates.
//   tiles   one workgroup of 256 lanes owns a box of tile[0] x tile[1] x tile[2] <= 256 nodes of the rank's sub-lattice, one node per
//           lane (z fastest, the order of tid).  The shape comes from the host (cavity_tile_shape): the one that stages the fewest
//           candidates per node, i.e. the smallest (volume of the inflated tile box) / (nodes) — a bounding box as close to a cube
//           as the spacings and the sub-lattice allow.  It is a run-time argument; a lane finds its node with two integer divisions, once.
//           Workgroups are dealt to the tiles in the XCD-aware order of brick_select_v (brick.hpp): workgroup b takes slot
//           (b % 8) * (grid / 8) + b / 8, so every XCD's L2 serves a contiguous run of tiles whose inflated boxes overlap.
//   staging the cells that overlap the tile's bounding box inflated by rwalk (search radius; in list mode plus the drift since the
//           list build) are found by the cell rule of grid.hpp (cell_coord_any: owned AND halo cells, clamped to the grid), counted
//           into a cell table in LDS (batches of CAV_CELLS cells, block scan) and thereby flattened into one index space of container
//           entries.  Lanes read consecutive entries (consecutive addresses inside a cell: coalesced), keep an entry iff it lies in
//           the GLOBAL box (0 <= r < L in every dimension: countNeighbours' search box clamped to [0, L] and the region iterator's
//           lo <= r < hi — periodic images never count, halo copies received from a neighbouring rank do, and a molecule that drifted
//           out of the box between two list builds is seen exactly once, through its image) and inside the tile box inflated by
//           rfilter (a hair above R: no node of the tile can reach anything else), and compact the survivors with ballot + mbcnt and
//           ONE LDS counter bump per wave into the workgroup-wide arrays {x, y, z} FP64 + id.
//   id      needed for the reference's id clash only (countNeighbours skips an entry whose id equals the node's tid, :298): staged as
//           u32 in an array of its own (ids >= 2^32 as 0: tid lies in [1, 2^32 - 1]), read by the count loop ONLY behind dd < RR.
//   chunks  a chunk is up to P.chunk consecutive ENTRIES of the flat index space (not survivors: then a chunk can never overflow and
//           staging needs no barrier of its own): stage, barrier, count, barrier, next chunk — any density, radius and spacing is
//           served by the one kernel; coarse lattices merely stage wastefully.  The fill counter alternates between two LDS words so
//           that it is cleared outside the window in which it is bumped.
//   count   every lane walks the staged survivors; all lanes of a wave read the same LDS address (broadcast, no bank conflicts).
//           dd = dx dx + dy dy + dz dz in FP64 in that order (MoleculeInterface.h:157-164; contraction off), dd < RR, id != tid.
//           Flag mode: a node is decided once count > maxNeighbours; a wave whose nodes are all decided (ballot, every 8 survivors)
//           skips the rest of the counting but keeps staging and meeting the barriers; when no wave has an undecided node left
//           (__syncthreads_or at the chunk's second barrier) the workgroup is done.  Count mode: no early exit, exact u32 counts.
//           One node per lane: a pair test is 8 FP64 operations (4 cycles each per wave) against three broadcast LDS reads, so the
//           loop is bound by the FP64 pipe, not by LDS — a second node per lane would halve what is not the limit; not built.
//   output  u8 flag (count <= maxNeighbours) per node in tid order of the sub-lattice, u32 counts in count mode, the number of active
//           nodes by wave ballot + popcount, one LDS atomic per wave and ONE u64 global atomic per workgroup.  Integer atomics only:
//           bitwise reproducible for a given state.
// LDS per workgroup: CAV_CAP = 1024 survivors x 28 B (3 doubles + u32 id) = 28 672 B, cell table 2 x CAV_CELLS x 4 B + 4 = 4 100 B, scan
// scratch and counters 28 B: 32.8 KB, i.e. four workgroups (16 waves, 4 per SIMD: the occupancy aimed at — the count loop has no
// global loads to hide) on the 160 KB of a gfx950 CU; a region of 125 cells at 7 molecules per cell fits one chunk.  Registers of the
// shipped build: the table at launch_cavity.
#include "common.hpp"
#include "brick.hpp"

namespace ls1 {

constexpr int CTPB = 256;
constexpr int CAV_CAP = 1024;    // entries of a staging chunk
constexpr int CAV_CELLS = 512;   // cells of a table batch (block_scan_lds: <= 4 x CTPB)
constexpr int CAV_CHECK = 8;     // survivors between two "is this wave decided" ballots

size_t cavity_chunk_max() { return (size_t)CAV_CAP; }

// the series word of this sample: cleared by a kernel of its own (no memset node, should a caller ever capture the pass)
__global__ void k_cavity_clear(unsigned long long* w) { *w = 0ull; }

template <bool COUNTS>
__global__ void __launch_bounds__(CTPB) k_cavity(CavityParams P) {
	__shared__ double sr[3 * CAV_CAP];     // survivors {x, y, z}
	__shared__ uint32_t sid[CAV_CAP];      // their ids (0: cannot clash)
	__shared__ uint32_t cstart[CAV_CELLS + 1];
	__shared__ uint32_t gbeg[CAV_CELLS];
	__shared__ uint32_t wsum[CTPB / 64];
	__shared__ uint32_t fill[2];
	__shared__ uint32_t s_active;

	const uint32_t t = threadIdx.x, lane = t & 63u;
	const uint32_t slot = (blockIdx.x % 8u) * (gridDim.x / 8u) + blockIdx.x / 8u;
	if (slot >= P.ntiles) return;  // uniform per workgroup
	if (t == 0) {
		fill[0] = fill[1] = 0u;
		s_active = 0u;
	}
	// ---- the tile and this lane's node -------------------------------------------------------------------------------------------
	const uint32_t tc[3] = {slot / (P.nt[2] * P.nt[1]), (slot / P.nt[2]) % P.nt[1], slot % P.nt[2]};
	const uint32_t ln[3] = {t / (P.tile[2] * P.tile[1]), (t / P.tile[2]) % P.tile[1], t % P.tile[2]};
	uint32_t first[3], ext[3];  // first node (sub-lattice index) and extent of the tile (partial at the upper faces)
	double flo[3], fhi[3], wlo[3], whi[3], pr[3];
	int c0[3], nc[3];
	bool own = true;
	for (int d = 0; d < 3; ++d) {
		first[d] = tc[d] * P.tile[d];
		ext[d] = min(P.tile[d], P.n[d] - first[d]);
		own = own && ln[d] < ext[d];
		// tq = control_bottom + (0.5009756 + tlu) * grid_spacing, CavityEnsemble.cpp:171
		const double a = P.cb[d] + (0.5009756 + (double)(P.lo[d] + first[d])) * P.h[d];
		const double b = P.cb[d] + (0.5009756 + (double)(P.lo[d] + first[d] + ext[d] - 1u)) * P.h[d];
		pr[d] = P.cb[d] + (0.5009756 + (double)(P.lo[d] + first[d] + min(ln[d], ext[d] - 1u))) * P.h[d];
		flo[d] = a - P.rfilter;
		fhi[d] = b + P.rfilter;
		wlo[d] = a - P.rwalk;
		whi[d] = b + P.rwalk;
		c0[d] = cell_coord_any(P.g, d, wlo[d]);
		nc[d] = cell_coord_any(P.g, d, whi[d]) - c0[d] + 1;  // cell_coord_any is monotone and stays inside [0, dims)
	}
	const uint64_t node = ((uint64_t)(first[0] + ln[0]) * P.n[1] + (first[1] + ln[1])) * P.n[2] + (first[2] + ln[2]);  // sub-lattice order
	// tid of the node (:169); <= 2^32 - 1 by ls1hip_cavity_config
	const uint32_t tid = (uint32_t)(((uint64_t)(P.lo[0] + first[0] + ln[0]) * P.N[1] + (P.lo[1] + first[1] + ln[1])) * P.N[2] +
									(P.lo[2] + first[2] + ln[2]) + 1ull);
	const double RR = P.RR;
	const uint32_t max_nb = P.max_nb;
	uint32_t cnt = 0;
	uint32_t par = 0;  // which fill word this chunk bumps
	bool done = false;

	const long ncell = (long)nc[0] * nc[1] * nc[2];
	for (long cb0 = 0; cb0 < ncell && !done; cb0 += CAV_CELLS) {
		// ---- cell table of this batch: counts -> exclusive prefix = the flat index space of its container entries -------------------
		const int nb = (int)min((long)CAV_CELLS, ncell - cb0);
		for (int c = (int)t; c < nb; c += CTPB) {
			const long rc = cb0 + c;
			const int rx = (int)(rc % nc[0]), ry = (int)((rc / nc[0]) % nc[1]), rz = (int)(rc / ((long)nc[0] * nc[1]));
			const int gc = cell_index(P.g, c0[0] + rx, c0[1] + ry, c0[2] + rz);
			const uint32_t beg = P.cell_begin[gc];
			gbeg[c] = beg;
			cstart[c] = P.cell_end[gc] - beg;
		}
		__syncthreads();
		block_scan_lds<CTPB>(cstart, nb, wsum);
		const uint32_t total = cstart[nb];
		for (uint32_t s = 0; s < total; s += P.chunk) {
			// ---- stage: entries [s, e) -> survivors ----------------------------------------------------------------------------------
			const uint32_t e = min(s + P.chunk, total);
			for (uint32_t r0 = s; r0 < e; r0 += CTPB) {  // uniform trip count: every lane takes part in the ballot
				const uint32_t r = r0 + t;
				bool keep = false;
				double x = 0., y = 0., z = 0.;
				uint32_t g = 0;
				if (r < e) {
					int lo = 0, hi = nb;
					while (hi - lo > 1) {
						const int mid = (lo + hi) >> 1;
						if (cstart[mid] <= r) lo = mid;
						else hi = mid;
					}
					g = gbeg[lo] + (r - cstart[lo]);
					x = P.x[g]; y = P.y[g]; z = P.z[g];
					keep = (x >= 0.) & (x < P.glen[0]) & (y >= 0.) & (y < P.glen[1]) & (z >= 0.) & (z < P.glen[2]) &  //
						   (x >= flo[0]) & (x <= fhi[0]) & (y >= flo[1]) & (y <= fhi[1]) & (z >= flo[2]) & (z <= fhi[2]);
				}
				const uint64_t m = __ballot(keep);
				if (m) {  // uniform per wave: one counter bump per wave and round
					const int leader = __ffsll((long long)m) - 1;
					uint32_t b = 0;
					if ((int)lane == leader) b = atomicAdd(&fill[par], (uint32_t)__popcll(m));
					b = __shfl(b, leader);
					if (keep) {
						const uint32_t k = b + lanes_below(m);  // < e - s <= CAV_CAP
						const uint64_t id = P.id[g];
						sr[3 * k] = x; sr[3 * k + 1] = y; sr[3 * k + 2] = z;
						sid[k] = id >> 32 ? 0u : (uint32_t)id;
					}
				}
			}
			__syncthreads();
			const uint32_t n = fill[par];
			if (t == 0) fill[par ^ 1u] = 0u;  // last read before the previous chunk's second barrier, next bumped behind this chunk's
			par ^= 1u;
			// ---- count: every lane against every survivor, broadcast reads ---------------------------------------------------------------
			for (uint32_t k0 = 0; k0 < n; k0 += CAV_CHECK) {
				if (!COUNTS && __ballot(own && cnt <= max_nb) == 0ull) break;  // every node of this wave is decided
				const uint32_t k1 = min(k0 + (uint32_t)CAV_CHECK, n);
				for (uint32_t k = k0; k < k1; ++k) {
					const double dx = sr[3 * k] - pr[0], dy = sr[3 * k + 1] - pr[1], dz = sr[3 * k + 2] - pr[2];
					const double dd = dx * dx + dy * dy + dz * dz;
					if (dd < RR) cnt += sid[k] != tid ? 1u : 0u;
				}
			}
			if constexpr (COUNTS) {
				__syncthreads();
			} else if (!__syncthreads_or(own && cnt <= max_nb)) {
				done = true;  // uniform: no undecided node left in the workgroup
				break;
			}
		}
	}
	// ---- output ------------------------------------------------------------------------------------------------------------------------
	const bool active = own && cnt <= max_nb;  // decideActivity, CavityEnsemble.cpp:254-259 (max_nb >= 1 by configuration)
	if (own) {
		P.flags[node] = active ? 1 : 0;
		if (COUNTS) P.counts[node] = cnt;
	}
	const uint64_t am = __ballot(active);
	if (lane == 0 && am) atomicAdd(&s_active, (uint32_t)__popcll(am));
	__syncthreads();
	if (t == 0 && s_active) atomicAdd(P.n_active, (unsigned long long)s_active);
}

// The tile shape that stages the fewest candidates per node: the candidates of a tile are the molecules inside its bounding box
// inflated by R, and every one of them is tested by all 256 lanes whether they own a node or not — so the cost per node is
// ((a - 1) h0 + 2R)((b - 1) h1 + 2R)((c - 1) h2 + 2R) / (a b c) over the shapes with a b c <= 256 that the sub-lattice can fill.  For equal spacings
// that is the most cubic box; the largest c for given a, b is always best.
void cavity_tile_shape(const uint32_t n[3], const double h[3], double R, uint32_t tile[3]) {
	double best = 0.;
	tile[0] = tile[1] = tile[2] = 1;
	for (uint32_t a = 1; a <= std::min<uint32_t>(CTPB, n[0]); ++a)
		for (uint32_t b = 1; b <= std::min<uint32_t>(CTPB / a, n[1]); ++b) {
			const uint32_t c = std::min<uint32_t>(CTPB / (a * b), n[2]);
			const double cost = ((a - 1) * h[0] + 2 * R) * ((b - 1) * h[1] + 2 * R) * ((c - 1) * h[2] + 2 * R) / ((double)a * b * c);
			if (best == 0. || cost < best) {
				best = cost;
				tile[0] = a; tile[1] = b; tile[2] = c;
			}
		}
}

// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), VGPRs / SGPRs / LDS per workgroup / waves per SIMD (the LDS bound):
//   k_cavity<false> (flag mode)   73 / 106 / 33 056 B / 4     no scratch, no VGPR spills (8 SGPRs spilled to VGPR lanes)
//   k_cavity<true>  (count mode)  72 / 106 / 32 800 B / 4     no scratch, no spills
void launch_cavity(const CavityParams& p, hipStream_t s) {
	hipLaunchKernelGGL(k_cavity_clear, dim3(1), dim3(1), 0, s, p.n_active);
	const dim3 grid(8u * ((p.ntiles + 7u) / 8u)), block(CTPB);  // multiple of 8: the XCD-aware order
	if (p.counts) hipLaunchKernelGGL(k_cavity<true>, grid, block, 0, s, p);
	else hipLaunchKernelGGL(k_cavity<false>, grid, block, 0, s, p);
}

}  // namespace ls1
