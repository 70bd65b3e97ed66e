// kernels_odf.hip — orientation distribution functions sampled on the device: the traversal of the linked cells that the reference's
// ODF plugin runs after the forces (io/ODF.cpp:81-85,123-331, adapter/ODFCellProcessor.cpp:16-92).
//
//   * brick-tiled like k_rdf_brick: one 256-thread workgroup per brick of BX x BY x BZ cells, the brick and its one-cell shell staged
//     ONCE into LDS in region-linear order.  Staged per molecule: centre FP64 x y z, molecule id, component id, and the orientation
//     vector e = (2(qx qz + qw qy), 2(qy qz - qw qx), 1 - 2(qx^2 + qy^2)) of the quaternion AS STORED (ODFCellProcessor.cpp:87-92,
//     ODF.cpp:191-193: not normalised), formed once per molecule here instead of once per pair.  A halo copy takes its quaternion from
//     its source molecule (between two list builds only halo positions are refreshed).  A molecule whose component does not have
//     exactly one dipole (ODFCellProcessor.cpp:25,34) is marked (component byte 0xff) and never becomes i or j;
//   * phase 1, the scan: one lane per owned molecule walks the nine neighbour rows, ODF_QSTEP candidates per scan step; the test is
//     dd < min(rc^2, shell^2), id_i < id_j, both marked — every unordered pair once in the sum over all ranks, as in the RDF pass.
//     A hit is NOT kept by its lane: it is appended as the slot pair (i, j), two u16, to ONE workgroup-wide queue in LDS; the queue
//     slot is the wave's ballot prefix on top of one LDS counter bump per wave and candidate.  About one candidate in twelve is a hit
//     at shell = r_c (one in fifty at 0.6 r_c): per-lane lists as in k_rdf_brick would leave most lanes idle in the expensive part;
//   * phase 2, the orientation math: when the queue cannot take another full scan step of the workgroup (256 lanes x ODF_QSTEP), and
//     at the end, all 256 lanes drain it, one hit per lane: dd again from the staged positions (the same expression: the same bits),
//     d^ = d / sqrt(dd), cos phi_1 = d^.e_i, cos phi_2 = -d^.e_j, p_k = d^ x (e_k x d^) normalised, cos gamma = p^_i.p^_j, the three
//     rounding rules (ODF.cpp:234-242), gamma = acos;
//   * bins: closed forms floor((1 - c) P / 2) and floor(gamma G / pi), then settled against the edge expressions of the reference's
//     search loop (ODF.cpp:253-270) themselves, so the index is the loop's for EVERY value; c == -1 -> P - 1, gamma == pi -> G
//     (:272-290), a value that fits nowhere (NaN: e parallel to d^) keeps index 0 as the reference leaves it;
//   * two words per pair: H[a][b][idx(i1, i2, g)] and H[b][a][idx(i2, i1, g)], a = cid_i, b = cid_j in {0, 1} (ODF.cpp:305-329),
//     idx = i1 P G + i2 G + g inside an array of W = P P G + 1 words, arrays in the order 11 12 21 22;
//   * counts go to a u32 histogram in LDS whose non-zero words are added to the global u64 arrays at the end; four arrays beyond the
//     budget go straight to global u64 atomics (same counts, slower).  Integer atomics only: bitwise reproducible.
// LDS per workgroup, budget 80 KB = two workgroups on the 160 KB of a gfx950 CU:
//   staging    ODF_CAPJ = 960 molecules x 57 B (3 + 3 doubles, id, component byte)            53.4 KB
//   hit queue  ODF_QCAP = 1536 entries x 4 B (drained above 1536 - 256 x ODF_QSTEP = 512)      6.0 KB
//   histogram  ODF_LDS_WORDS = 4096 u32: 4 W <= 4096, e.g. 10 x 10 x 10 increments            16.0 KB
//   cell tables, scan scratch, queue counters (4 x 4 x 4 bricks)                               2.0 KB
#include "common.hpp"
#include "brick.hpp"

namespace ls1 {

constexpr int OTPB = 256;
constexpr int ODF_CAPJ = 960;
constexpr int ODF_QSTEP = 4;
constexpr int ODF_QCAP = 1536;
constexpr int ODF_LDS_WORDS = 4096;
constexpr uint8_t ODF_NOT_DIPOLAR = 0xff;
static_assert(ODF_QCAP > OTPB * ODF_QSTEP && ODF_CAPJ < 65536, "queue: room for one scan step of the workgroup, u16 slots");

size_t odf_lds_words() { return (size_t)ODF_LDS_WORDS; }

// ODFCellProcessor::calcOrientationVector (ODFCellProcessor.cpp:87-92) = ODF.cpp:191-193, from (qw, qx, qy, qz) as stored
__device__ __forceinline__ void odf_evec(double w, double x, double y, double z, double& ex, double& ey, double& ez) {
	ex = 2 * (x * z + w * y);
	ey = 2 * (y * z - w * x);
	ez = 1 - 2 * (x * x + y * y);
}

// the i of ODF.cpp:253-264 with 1 - 2 i / P >= c > 1 - 2 (i + 1) / P; c == -1 -> P - 1 (:277-285); nothing fits -> 0
__device__ __forceinline__ uint32_t odf_cos_bin(double c, int P) {
	if (!(c <= 1. && c >= -1.)) return 0u;
	const double p = (double)P;
	int i = (int)fmin(floor((1. - c) * p / 2.), p - 1.);
	if (i > 0 && !(1. - i * 2. / p >= c)) --i;
	else if (i < P - 1 && !(c > 1. - (i + 1) * 2. / p)) ++i;
	return (uint32_t)i;
}

// i + 1 for the i of ODF.cpp:266-269 with i pi / G <= gamma < (i + 1) pi / G; gamma == pi -> G (:272-274,287-290); NaN -> 0
__device__ __forceinline__ uint32_t odf_gamma_bin(double gam, int G) {
	if (!(gam >= 0. && gam <= M_PI)) return 0u;
	const double g = (double)G;
	int i = (int)fmin(floor(gam * g / M_PI), g - 1.);
	if (i > 0 && !(i * M_PI / g <= gam)) --i;
	else if (i < G - 1 && !(gam < (i + 1) * M_PI / g)) ++i;
	return (uint32_t)i + 1u;
}

__device__ __forceinline__ double odf_round_rule(double c) {  // ODF.cpp:234-242, roundingThreshold = 0.0001
	return (fabs(c) < 0.0001 || fabs(fabs(c) - 1.) < 0.0001) ? round(c) : c;
}

// ODF::calculateOrientation (ODF.cpp:184-306) for d = r_j - r_i (halo image of j), dd = |d|^2 < shell^2: the word offsets
// idx(i1, i2, g) and idx(i2, i1, g) inside an array
__device__ __forceinline__ void odf_orientation(double dx, double dy, double dz, double dd, double e1x, double e1y, double e1z, double e2x,
												 double e2y, double e2z, int P, int G, uint32_t& el, uint32_t& rev) {
	const double r = sqrt(dd);
	dx /= r; dy /= r; dz /= r;
	const double a1x = e1y * dz - e1z * dy, a1y = e1z * dx - e1x * dz, a1z = e1x * dy - e1y * dx;
	double p1x = dy * a1z - dz * a1y, p1y = dz * a1x - dx * a1z, p1z = dx * a1y - dy * a1x;
	const double a2x = e2y * dz - e2z * dy, a2y = e2z * dx - e2x * dz, a2z = e2x * dy - e2y * dx;
	double p2x = dy * a2z - dz * a2y, p2y = dz * a2x - dx * a2z, p2z = dx * a2y - dy * a2x;
	double c1 = dx * e1x + dy * e1y + dz * e1z;
	double c2 = -(dx * e2x + dy * e2y + dz * e2z);
	const double n1 = sqrt(p1x * p1x + p1y * p1y + p1z * p1z), n2 = sqrt(p2x * p2x + p2y * p2y + p2z * p2z);
	p1x /= n1; p1y /= n1; p1z /= n1;
	p2x /= n2; p2y /= n2; p2z /= n2;
	double cg = p1x * p2x + p1y * p2y + p1z * p2z;
	c1 = odf_round_rule(c1);
	c2 = odf_round_rule(c2);
	cg = odf_round_rule(cg);
	const uint32_t i1 = odf_cos_bin(c1, P), i2 = odf_cos_bin(c2, P), g = odf_gamma_bin(acos(cg), G);
	el = (i1 * (uint32_t)P + i2) * (uint32_t)G + g;
	rev = (i2 * (uint32_t)P + i1) * (uint32_t)G + g;
}

template <int BX, int BY, int BZ>
__global__ void __launch_bounds__(OTPB) k_odf_brick(ForceParams P, OdfParams O, int has_rot, int nbx, int nby, int nbz) {
	constexpr int HW = 1, NT = OTPB, CAPJ = ODF_CAPJ;
	constexpr int RX = BX + 2 * HW, RY = BY + 2 * HW, RZ = BZ + 2 * HW;
	constexpr int NRC = RX * RY * RZ;
	constexpr int NBC = BX * BY * BZ;
	constexpr int NW = 3, NROWS = 9;
	__shared__ double sx[CAPJ], sy[CAPJ], sz[CAPJ];
	__shared__ double ox[CAPJ], oy[CAPJ], oz[CAPJ];  // orientation vector e
	__shared__ uint64_t sid[CAPJ];
	__shared__ uint8_t scid[CAPJ];  // component id (0 or 1) of a single-dipole molecule, ODF_NOT_DIPOLAR otherwise
	__shared__ uint32_t queue[ODF_QCAP];  // hits: i slot | j slot << 16
	__shared__ uint32_t qc[3];            // hits appended in scan step s, at [s % 3]
	__shared__ uint32_t cstart[NRC + 1];
	__shared__ uint32_t gbeg[NRC];
	__shared__ uint32_t bstart[NBC + 1];
	__shared__ uint32_t wsum[NT / 64];
	__shared__ uint32_t hist[ODF_LDS_WORDS];

	const int tid = threadIdx.x;
	const BrickSel bs = brick_select<HW, BX, BY, BZ>(P, nbx, nby, nbz);
	if (!bs.live) return;  // uniform per workgroup
	const uint32_t W = O.W, lds_words = O.hist_lds ? 4u * W : 0u;  // <= ODF_LDS_WORDS (launch_odf)
	for (uint32_t w = tid; w < lds_words; w += NT) hist[w] = 0u;
	if (tid < 3) qc[tid] = 0u;
	// ---- region cell table, brick cell prefix --------------------------------------------------------------------------
	uint32_t total, n_i;
	brick_prefixes<NT, HW, BX, BY, BZ>(P, bs, cstart, gbeg, bstart, wsum, total, n_i);
	const bool staged = total <= (uint32_t)CAPJ;
	const uint32_t n_real = P.cnt->n_real;
	const uint32_t mask = O.dip_mask;
	// orientation vector of slot g: a halo image takes the quaternion of its source molecule — between two builds of the neighbour
	// lists only the POSITIONS of the halo copies are refreshed, the owned molecules' orientations are always current
	auto evec = [&](uint32_t g, double& vx, double& vy, double& vz) {
		vx = 0.; vy = 0.; vz = 1.;
		if (!has_rot) return;  // (no component has a dipole then: nothing is marked)
		g = halo_source_slot(g, n_real, O.hsrc);
		odf_evec(P.q0[g], P.q1[g], P.q2[g], P.q3[g], vx, vy, vz);
	};
	auto comp_byte = [&](int c) { return ((mask >> c) & 1u) ? (uint8_t)c : ODF_NOT_DIPOLAR; };
	if (staged) {
		for (uint32_t s = tid; s < total; s += NT) {
			const int lo = slot_cell(cstart, NRC, s);
			const uint32_t g = gbeg[lo] + (s - cstart[lo]);
			sx[s] = P.x[g];
			sy[s] = P.y[g];
			sz[s] = P.z[g];
			sid[s] = O.id[g];
			const uint8_t cb = comp_byte(P.cid[g]);
			scid[s] = cb;
			double vx = 0., vy = 0., vz = 1.;
			if (cb != ODF_NOT_DIPOLAR) evec(g, vx, vy, vz);
			ox[s] = vx; oy[s] = vy; oz[s] = vz;
		}
	}
	__syncthreads();

	const double cut2 = O.cut2;
	const int NP = O.P, NG = O.G;
	// one pair inside the shell: ODF::calculateOrientation's two increments (ODF.cpp:305-329)
	auto observe = [&](double dx, double dy, double dz, double dd, int a, double e1x, double e1y, double e1z, int b, double e2x, double e2y,
					   double e2z) {
		uint32_t el, rev;
		odf_orientation(dx, dy, dz, dd, e1x, e1y, e1z, e2x, e2y, e2z, NP, NG, el, rev);
		const uint32_t w1 = (uint32_t)(a * 2 + b) * W + el, w2 = (uint32_t)(b * 2 + a) * W + rev;
		if (O.hist_lds) {
			atomicAdd(&hist[w1], 1u);
			atomicAdd(&hist[w2], 1u);
		} else {
			atomicAdd(&O.g_hist[w1], 1ull);
			atomicAdd(&O.g_hist[w2], 1ull);
		}
	};

	const uint32_t lane = (uint32_t)tid & 63u;
	uint32_t qfill = 0, step = 0;  // entries in the queue, scan steps done: both uniform over the workgroup
	for (uint32_t base = 0; base < n_i; base += NT) {  // one pass unless the brick holds more than 256 molecules
		const uint32_t it = base + (uint32_t)tid;
		bool act = it < n_i;
		uint32_t ii = 0, gi = 0;
		int rowbase = 0;
		if (act) {
			const BrickOwned o = brick_owned<HW, BX, BY, BZ>(cstart, gbeg, bstart, it);
			ii = o.ii; gi = o.gi; rowbase = o.rowbase;
		}
		if (staged) {
			act = act && scid[ii] != ODF_NOT_DIPOLAR;
			const double xi = act ? sx[ii] : 0., yi = act ? sy[ii] : 0., zi = act ? sz[ii] : 0.;
			const uint64_t idi = act ? sid[ii] : 0ull;
			int row = act ? 0 : NROWS;
			uint32_t j = 0, je = 0;
			for (;;) {  // scan steps: every thread of the workgroup takes part in every one (barriers)
				const uint32_t slot = step % 3u;
#pragma unroll
				for (int k = 0; k < ODF_QSTEP; ++k) {
					while (j >= je && row < NROWS) {
						const int r0 = rowbase + (row / NW) * (RY * RX) + (row % NW) * RX;
						j = cstart[r0];
						je = cstart[r0 + NW];
						++row;
					}
					const bool valid = j < je;
					bool hit = false;
					if (valid) {
						const double dx = sx[j] - xi, dy = sy[j] - yi, dz = sz[j] - zi;
						const double dd = dx * dx + dy * dy + dz * dz;
						hit = (dd < cut2) & (idi < sid[j]) & (scid[j] != ODF_NOT_DIPOLAR);
					}
					const unsigned long long m = __ballot(hit);
					if (m) {  // uniform per wave: one counter bump per wave and candidate
						const int leader = __ffsll((long long)m) - 1;
						uint32_t b = 0;
						if ((int)lane == leader) b = atomicAdd(&qc[slot], (uint32_t)__popcll(m));
						b = __shfl(b, leader);
						if (hit) queue[qfill + b + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = ii | (j << 16);
					}
					j += valid ? 1u : 0u;
				}
				const int more = (j < je) | (row < NROWS);
				const int any = __syncthreads_or(more);
				// qc[slot] is final: step s + 1 counts in another word, and this word is cleared two steps on, after the barrier
				// behind which every thread has read it
				qfill += qc[slot];
				if (tid == 0) qc[(step + 2u) % 3u] = 0u;
				++step;
				if (!any || qfill > (uint32_t)(ODF_QCAP - NT * ODF_QSTEP)) {
					for (uint32_t q = tid; q < qfill; q += NT) {  // phase 2: one hit per lane
						const uint32_t e = queue[q], a = e & 0xffffu, b = e >> 16;
						const double dx = sx[b] - sx[a], dy = sy[b] - sy[a], dz = sz[b] - sz[a];
						const double dd = dx * dx + dy * dy + dz * dz;  // the same expression as in the scan: the same bits
						observe(dx, dy, dz, dd, (int)scid[a], ox[a], oy[a], oz[a], (int)scid[b], ox[b], oy[b], oz[b]);
					}
					qfill = 0;
					__syncthreads();  // the queue is free again
				}
				if (!any) break;
			}
		} else if (act) {
			// shell does not fit the staging area: same arithmetic straight from global memory, no queue
			const uint8_t ca = comp_byte(P.cid[gi]);
			if (ca == ODF_NOT_DIPOLAR) continue;
			const double xi = P.x[gi], yi = P.y[gi], zi = P.z[gi];
			const uint64_t idi = O.id[gi];
			double e1x, e1y, e1z;
			evec(gi, e1x, e1y, e1z);
			for (int row = 0; row < NROWS; ++row) {
				const int r0 = rowbase + (row / NW) * (RY * RX) + (row % NW) * RX;
				for (int c = r0; c < r0 + NW; ++c) {
					const uint32_t g0 = gbeg[c], n = cstart[c + 1] - cstart[c];
					for (uint32_t j = g0; j < g0 + n; ++j) {
						const double dx = P.x[j] - xi, dy = P.y[j] - yi, dz = P.z[j] - zi;
						const double dd = dx * dx + dy * dy + dz * dz;
						if (!((dd < cut2) & (idi < O.id[j]))) continue;
						const uint8_t cb = comp_byte(P.cid[j]);
						if (cb == ODF_NOT_DIPOLAR) continue;
						double e2x, e2y, e2z;
						evec(j, e2x, e2y, e2z);
						observe(dx, dy, dz, dd, (int)ca, e1x, e1y, e1z, (int)cb, e2x, e2y, e2z);
					}
				}
			}
		}
	}
	__syncthreads();
	// ---- flush: non-zero words of the workgroup's histogram -> global u64 arrays ------------------------------------------------------
	for (uint32_t w = tid; w < lds_words; w += NT) {
		const uint32_t v = hist[w];
		if (v) atomicAdd(&O.g_hist[w], (unsigned long long)v);
	}
}

template <int BX, int BY, int BZ>
static bool launch_odf_shape(ForceParams p, const OdfParams& o, bool has_rot, hipStream_t s) {
	int nbx, nby, nbz;
	const dim3 grid(all_bricks_grid<BX, BY, BZ>(p, nbx, nby, nbz)), block(OTPB);
	if (!grid.x) return false;
	hipLaunchKernelGGL((k_odf_brick<BX, BY, BZ>), grid, block, 0, s, p, o, has_rot ? 1 : 0, nbx, nby, nbz);
	return true;
}

// The brick shape follows the mean cell occupancy as in launch_rdf: the largest shape whose shell fits the staging area with 8 %
// headroom; a brick whose shell overflows all the same walks global memory (same arithmetic, same counts).
bool launch_odf(const ForceParams& p, OdfParams o, bool has_rot, double mean_per_cell, hipStream_t s) {
	if (p.g.hw != 1) return false;
	o.hist_lds = 4 * (size_t)o.W <= (size_t)ODF_LDS_WORDS;
	const double m = mean_per_cell * 1.08, cap = (double)ODF_CAPJ;
	if (m * (6 * 6 * 6) <= cap) return launch_odf_shape<4, 4, 4>(p, o, has_rot, s);
	if (m * (6 * 6 * 4) <= cap) return launch_odf_shape<4, 4, 2>(p, o, has_rot, s);  // (4.4 molecules per cell: 141 of 256 lanes own one)
	if (m * (6 * 4 * 4) <= cap) return launch_odf_shape<4, 2, 2>(p, o, has_rot, s);
	return launch_odf_shape<2, 2, 2>(p, o, has_rot, s);
}

}  // namespace ls1
