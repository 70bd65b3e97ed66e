// kernels_ardf.hip — the angular RDF sampled on the device: distance x cos(phi) histograms of the reference's RDF plugin with
// angularbins > 1 (io/RDF.h:93-109 observeARDFMolecule, adapter/RDFCellProcessor.cpp:36-41, MoleculeInterface.h:167-190
// orientationAngle), in the cell traversal of the RDF pass.
//
//   * pairs: the rule of kernels_rdf.hip — (i owned, j owned or halo image) is observed by i iff id_i < id_j and dd < rc^2, dd of
//     d = r_j - r_i; a molecule's own periodic image is never a pair.  Every observed pair adds TWO counts:
//     ardf[c_i][c_j][flat(b, a_ij)] and ardf[c_j][c_i][flat(b, a_ji)]; the first index is the component of the CENTRAL molecule, the
//     histogram of nC x nC x (bins A) words is not symmetric;
//   * arithmetic, operation for operation the reference's: orientation vector of the quaternion (w, x, y, z) AS STORED
//     o = (2.(xz + wy), 2.(yz - wx), 1. - 2.(xx + yy)), s = sqrt(((0 + o0 o0) + o1 o1) + o2 o2);
//     cos = ((0 + o0 d0 / s / sq) + o1 d1 / s / sq) + o2 d2 / s / sq with sq = sqrt(dd), every term ((o d) / s) / sq; the central
//     molecule i takes d, the central molecule j takes -d (exact).  IEEE sqrt and division, no contraction;
//   * bins: dd > (bins dr)^2 dropped, b = floor(sq / dr), b >= bins dropped; a = floor((-cos + 1.) / (2. / A));
//   * THE FLAT-INDEX QUIRK, kept: flat = b A + a in signed arithmetic (RDF.h:97-100).  a is -1 when cos rounds above 1 and A when
//     cos <= -1, and the count then lands in the neighbouring distance row (b - 1, column A - 1, or b + 1, column 0).  Only a flat
//     index outside [0, bins A) is dropped: the reference writes outside its vector there;
//   * components without rotation carry (1, 0, 0, 0): o = (0, 0, 1), s = 1 (the ROT = false kernels stage no orientation at all).
//
// Design.  One 256-thread workgroup per brick; brick and shell staged ONCE into LDS in region-linear order (brick_prefixes): x y z,
// id, component byte and, with ROT, o0 o1 o2 s evaluated once per molecule at staging (deterministic: the bits of the per-pair
// evaluation) from the quaternion of the halo image's source molecule — 65 B per molecule, 33 B without rotation.
// Walk: one lane per owned molecule over the 9 neighbour rows, all 64 lanes of a wave in step.  A hit is NOT kept by its lane: the
// wave compacts the hits of one step (ballot + prefix popcount) into its OWN queue of (i slot, j slot) u16 pairs in LDS; as soon as
// the queue holds 64 entries the wave drains 64 of them, one per lane, through the division chain (9 IEEE divisions, one sqrt, 2-3
// atomics per pair), and the tail at the end.  About one candidate in twelve is a hit, so binning inside the walk would leave 63
// lanes waiting, and per-lane lists (k_rdf_brick) leave the lanes with few hits idle in the expensive part.  The queues are
// per wave: between the barrier behind the staging and the one in front of the flush there is NO workgroup barrier (the ODF pass'
// workgroup-wide queue pays one per scan step); waves share the read-only staging area and the atomic histogram only.
// Histogram: u32 words in LDS, the non-zero ones added to the global u64 histogram at the end.  Budget ARDF_LDS_WORDS: ARDF words
// (plus the molecule words with MOL) fit -> all in LDS; only the molecule words fit -> they stay in LDS, ARDF counts go to global
// atomics; else everything goes to global atomics.  Integer atomics: every placement gives the same counts.
// MOL = true also bins mol[pair][b] and the per-component molecule counters of k_rdf_brick in the same walk (one traversal for an
// RDF + ARDF sample without site histograms).  A shell beyond the staging area walks global memory, same arithmetic.
//
// LDS per workgroup (<= 80 KB: two workgroups on the 160 KB of a gfx950 CU), 4 x 4 x 4 bricks:
//   staging ROT 600 x 65 B = 39 000 B (no rotation: 1200 x 33 B = 39 600 B), queues 4 x 128 x 4 B = 2 048 B, histogram
//   ARDF_LDS_WORDS x 4 B = 36 864 B, cell tables + counters 2 040 B.
// The compiler's resource usage for gfx950 (-Rpass-analysis=kernel-resource-usage), 4 x 4 x 4 bricks, the largest of the shapes:
//   with rotation    MOL / not   LDS 79 984 B   96 / 94 VGPRs   scratch 0
//   no rotation      MOL / not   LDS 80 576 B   72 / 72 VGPRs   scratch 0
#include "common.hpp"
#include "brick.hpp"

namespace ls1 {

constexpr int ATPB = 256;
constexpr int ARDF_LDS_WORDS = 9216;
constexpr int ARDF_QCAP = 128;  // a wave drains at 64: at most 63 + 64 entries
constexpr int ARDF_CAPJ_ROT = 600, ARDF_CAPJ_FIXED = 1200;

// MoleculeInterface::orientationAngle (MoleculeInterface.h:174-182): orientation vector and its length from (w, x, y, z) as stored
__device__ __forceinline__ void ardf_ovec(double w, double x, double y, double z, double& o0, double& o1, double& o2, double& s) {
	o0 = 2. * (x * z + w * y);
	o1 = 2. * (y * z - w * x);
	o2 = 1. - 2. * (x * x + y * y);
	s = sqrt(((0. + o0 * o0) + o1 * o1) + o2 * o2);
}
// ... and its cosine for d = r_other - r_central (MoleculeInterface.h:184-186)
__device__ __forceinline__ double ardf_cos(double o0, double o1, double o2, double s, double d0, double d1, double d2, double sq) {
	return ((0. + o0 * d0 / s / sq) + o1 * d1 / s / sq) + o2 * d2 / s / sq;
}
// RDF.h:97-100: flat = b A + a with a = floor((-cos + 1.) / aw) in {-1 ... A}, signed; b, a and the sum are small whole numbers, so
// the double arithmetic is exact.  false: outside [0, bins A) (or cos not a number), dropped
__device__ __forceinline__ bool ardf_flat(double cosphi, double b, const ArdfParams& A, uint32_t& flat) {
	const double a = floor((-cosphi + 1.) / A.aw);
	const double f = b * (double)A.abins + a;
	if (!(f >= 0. && f < (double)A.pair_words)) return false;
	flat = (uint32_t)f;
	return true;
}

template <int BX, int BY, int BZ, int CAPJ, bool ROT, bool MOL>
__global__ void __launch_bounds__(ATPB) k_ardf_brick(ForceParams P, RdfParams R, ArdfParams A, int nbx, int nby, int nbz) {
	constexpr int HW = 1, NT = ATPB, NWAVE = NT / 64;
	constexpr int RX = BX + 2 * HW, RY = BY + 2 * HW, RZ = BZ + 2 * HW;
	constexpr int NRC = RX * RY * RZ;
	constexpr int NBC = BX * BY * BZ;
	constexpr int NW = 3, NROWS = 9;
	constexpr int ON = ROT ? CAPJ : 1;
	static_assert(CAPJ < 65536, "queue entries hold u16 slots");
	static_assert(CAPJ * (33 + (ROT ? 32 : 0)) + NWAVE * ARDF_QCAP * 4 + ARDF_LDS_WORDS * 4 + (2 * NRC + NBC + 2 + NWAVE + MAXC) * 4 <= 80 * 1024,
				  "two workgroups per CU");
	__shared__ double sx[CAPJ], sy[CAPJ], sz[CAPJ];
	__shared__ double so0[ON], so1[ON], so2[ON], ss[ON];  // orientation vector and its length
	__shared__ uint64_t sid[CAPJ];
	__shared__ uint8_t scid[CAPJ];
	__shared__ uint32_t queue[NWAVE][ARDF_QCAP];  // per wave: hits as i slot | j slot << 16
	__shared__ uint32_t cstart[NRC + 1];
	__shared__ uint32_t gbeg[NRC];
	__shared__ uint32_t bstart[NBC + 1];
	__shared__ uint32_t wsum[NWAVE];
	__shared__ uint32_t hist[ARDF_LDS_WORDS];
	__shared__ uint32_t ncnt[MAXC];

	const int tid = threadIdx.x;
	const BrickSel bs = brick_select<HW, BX, BY, BZ>(P, nbx, nby, nbz);
	if (!bs.live) return;  // uniform per workgroup
	const bool mol_lds = MOL && R.mol_lds;
	const uint32_t ardf_base = mol_lds ? R.mol_words : 0u;
	const uint32_t lds_words = ardf_base + (A.hist_lds ? A.words : 0u);  // <= ARDF_LDS_WORDS (launch_ardf)
	for (uint32_t w = tid; w < lds_words; w += NT) hist[w] = 0u;
	if (tid < MAXC) ncnt[tid] = 0u;
	uint32_t total, n_i;
	brick_prefixes<NT, HW, BX, BY, BZ>(P, bs, cstart, gbeg, bstart, wsum, total, n_i);
	const bool staged = total <= (uint32_t)CAPJ;
	const uint32_t n_real = P.cnt->n_real;
	// orientation of slot g: a halo image takes the quaternion of its source molecule (only halo POSITIONS are refreshed between builds)
	auto ovec = [&](uint32_t g, double& o0, double& o1, double& o2, double& s) {
		o0 = 0.; o1 = 0.; o2 = 1.; s = 1.;  // (1, 0, 0, 0)
		if (!ROT) return;
		g = halo_source_slot(g, n_real, R.hsrc);
		ardf_ovec(P.q0[g], P.q1[g], P.q2[g], P.q3[g], o0, o1, o2, s);
	};
	if (staged) {
		for (uint32_t s = tid; s < total; s += NT) {
			const int lo = slot_cell(cstart, NRC, s);
			const uint32_t g = gbeg[lo] + (s - cstart[lo]);
			sx[s] = P.x[g];
			sy[s] = P.y[g];
			sz[s] = P.z[g];
			sid[s] = R.id[g];
			scid[s] = (uint8_t)P.cid[g];
			if (ROT) ovec(g, so0[s], so1[s], so2[s], ss[s]);
		}
	}
	__syncthreads();

	const double rc2 = R.rc2, maxd2 = R.maxd2, dr = R.dr;
	const double fbins = (double)R.bins;
	const uint32_t bins = (uint32_t)R.bins;
	const int ncomp = R.ncomp;
	auto add_ardf = [&](uint32_t w) {
		if (A.hist_lds) atomicAdd(&hist[ardf_base + w], 1u);
		else atomicAdd(&A.g_ardf[w], 1ull);
	};
	// one molecule pair inside the cutoff, d = r_j - r_i: RDF::observeRDFMolecule (MOL) and RDF::observeARDFMolecule
	auto observe = [&](double d0, double d1, double d2, double dd, int ci, double oi0, double oi1, double oi2, double si, int cj,
					   double oj0, double oj1, double oj2, double sj) {
		if (dd > maxd2) return;
		const double sq = sqrt(dd);
		const double b = floor(sq / dr);
		if (!(b < fbins)) return;
		if (MOL) {
			const int ca = min(ci, cj), cb = max(ci, cj);
			const uint32_t w = (uint32_t)(ca * ncomp - (ca * (ca - 1)) / 2 + (cb - ca)) * bins + (uint32_t)b;
			if (mol_lds) atomicAdd(&hist[w], 1u);
			else atomicAdd(&R.g_mol[w], 1ull);
		}
		const double cij = ardf_cos(oi0, oi1, oi2, si, d0, d1, d2, sq);
		const double cji = ardf_cos(oj0, oj1, oj2, sj, -d0, -d1, -d2, sq);
		uint32_t f;
		if (ardf_flat(cij, b, A, f)) add_ardf((uint32_t)(ci * ncomp + cj) * A.pair_words + f);
		if (ardf_flat(cji, b, A, f)) add_ardf((uint32_t)(cj * ncomp + ci) * A.pair_words + f);
	};

	const uint32_t lane = (uint32_t)tid & 63u;
	uint32_t* const q = queue[tid >> 6];
	uint32_t qn = 0;  // entries in this wave's queue: uniform over the wave
	// lanes 0 .. n - 1 take the entries first .. first + n - 1: dd again from the staged positions (the expression of the walk: its bits)
	auto drain = [&](uint32_t first, uint32_t n) {
		if (lane >= n) return;
		const uint32_t e = q[first + lane], a = e & 0xffffu, b = e >> 16;
		const double dx = sx[b] - sx[a], dy = sy[b] - sy[a], dz = sz[b] - sz[a];
		const double dd = dx * dx + dy * dy + dz * dz;
		if (ROT) observe(dx, dy, dz, dd, (int)scid[a], so0[a], so1[a], so2[a], ss[a], (int)scid[b], so0[b], so1[b], so2[b], ss[b]);
		else observe(dx, dy, dz, dd, (int)scid[a], 0., 0., 1., 1., (int)scid[b], 0., 0., 1., 1.);
	};
	for (uint32_t base = 0; base < n_i; base += NT) {  // one pass unless the brick holds more than 256 molecules
		const uint32_t it = base + (uint32_t)tid;
		const bool act = it < n_i;
		uint32_t ii = 0, gi = 0;
		int rowbase = 0;
		if (act) {
			const BrickOwned o = brick_owned<HW, BX, BY, BZ>(cstart, gbeg, bstart, it);
			ii = o.ii; gi = o.gi; rowbase = o.rowbase;
		}
		if (staged) {
			const double xi = sx[ii], yi = sy[ii], zi = sz[ii];
			const uint64_t idi = sid[ii];
			if (MOL && act) atomicAdd(&ncnt[scid[ii]], 1u);
			int row = act ? 0 : NROWS;
			uint32_t j = 0, je = 0;
			for (;;) {  // one candidate per lane and step; the lanes of a wave stay in step (ballots), the waves do not
				while (j >= je && row < NROWS) {
					const int r0 = rowbase + (row / NW) * (RY * RX) + (row % NW) * RX;
					j = cstart[r0];
					je = cstart[r0 + NW];
					++row;
				}
				const bool valid = j < je;
				if (__ballot(valid) == 0ull) break;
				bool hit = false;
				if (valid) {
					const double dx = sx[j] - xi, dy = sy[j] - yi, dz = sz[j] - zi;
					const double dd = dx * dx + dy * dy + dz * dz;
					hit = (dd < rc2) & (idi < sid[j]);
				}
				const uint64_t m = __ballot(hit);
				if (m) {
					if (hit) q[qn + lanes_below(m)] = ii | (j << 16);
					qn += (uint32_t)__popcll(m);
					if (qn >= 64u) {
						qn -= 64u;
						wave_lds_order();
						drain(qn, 64u);
						wave_lds_order();  // the drained slots are written again
					}
				}
				j += valid ? 1u : 0u;
			}
		} else if (act) {
			// shell does not fit the staging area: same arithmetic straight from global memory, no queue
			const double xi = P.x[gi], yi = P.y[gi], zi = P.z[gi];
			const int ci = P.cid[gi];
			const uint64_t idi = R.id[gi];
			double oi0, oi1, oi2, si;
			ovec(gi, oi0, oi1, oi2, si);
			if (MOL) atomicAdd(&ncnt[ci], 1u);
			for (int row = 0; row < NROWS; ++row) {
				const int r0 = rowbase + (row / NW) * (RY * RX) + (row % NW) * RX;
				for (int c = r0; c < r0 + NW; ++c) {
					const uint32_t g0 = gbeg[c], n = cstart[c + 1] - cstart[c];
					for (uint32_t j = g0; j < g0 + n; ++j) {
						const double dx = P.x[j] - xi, dy = P.y[j] - yi, dz = P.z[j] - zi;
						const double dd = dx * dx + dy * dy + dz * dz;
						if (!((dd < rc2) & (idi < R.id[j]))) continue;
						double oj0, oj1, oj2, sj;
						ovec(j, oj0, oj1, oj2, sj);
						observe(dx, dy, dz, dd, ci, oi0, oi1, oi2, si, P.cid[j], oj0, oj1, oj2, sj);
					}
				}
			}
		}
	}
	wave_lds_order();
	drain(0u, qn);  // the tail (qn < 64)
	__syncthreads();
	// ---- flush: non-zero words of the workgroup's histogram -> global u64 histograms -------------------------------------------------
	for (uint32_t w = tid; w < lds_words; w += NT) {
		const uint32_t v = hist[w];
		if (v == 0u) continue;
		if (w < ardf_base) atomicAdd(&R.g_mol[w], (unsigned long long)v);
		else atomicAdd(&A.g_ardf[w - ardf_base], (unsigned long long)v);
	}
	if (MOL && tid < ncomp && ncnt[tid]) atomicAdd(&R.g_n[tid], (unsigned long long)ncnt[tid]);
}

template <int BX, int BY, int BZ>
static bool launch_ardf_shape(ForceParams p, const RdfParams& r, const ArdfParams& a, bool mol, bool has_rot, hipStream_t s) {
	int nbx, nby, nbz;
	const dim3 grid(all_bricks_grid<BX, BY, BZ>(p, nbx, nby, nbz)), block(ATPB);
	if (!grid.x) return false;
	if (has_rot && mol) hipLaunchKernelGGL((k_ardf_brick<BX, BY, BZ, ARDF_CAPJ_ROT, true, true>), grid, block, 0, s, p, r, a, nbx, nby, nbz);
	else if (has_rot) hipLaunchKernelGGL((k_ardf_brick<BX, BY, BZ, ARDF_CAPJ_ROT, true, false>), grid, block, 0, s, p, r, a, nbx, nby, nbz);
	else if (mol) hipLaunchKernelGGL((k_ardf_brick<BX, BY, BZ, ARDF_CAPJ_FIXED, false, true>), grid, block, 0, s, p, r, a, nbx, nby, nbz);
	else hipLaunchKernelGGL((k_ardf_brick<BX, BY, BZ, ARDF_CAPJ_FIXED, false, false>), grid, block, 0, s, p, r, a, nbx, nby, nbz);
	return true;
}

// Staging capacity and brick shape follow launch_rdf: 600 molecules at 65 B with orientations, as its site variant; without rotation
// 1200 at 33 B (launch_rdf takes 1312 there: the 36 KB histogram takes the difference).  The largest shape whose shell fits with 8 %
// headroom; a brick whose shell overflows all the same walks global memory (same arithmetic, same counts).
bool launch_ardf(const ForceParams& p, RdfParams r, ArdfParams a, bool mol, bool has_rot, double mean_per_cell, hipStream_t s) {
	if (p.g.hw != 1) return false;
	const uint64_t mw = mol ? r.mol_words : 0u;
	r.mol_lds = mol && mw <= (uint64_t)ARDF_LDS_WORDS;
	a.hist_lds = mw + a.words <= (uint64_t)ARDF_LDS_WORDS;  // (then the molecule words fit too)
	const double m = mean_per_cell * 1.08, cap = has_rot ? (double)ARDF_CAPJ_ROT : (double)ARDF_CAPJ_FIXED;
	if (m * (6 * 6 * 6) <= cap) return launch_ardf_shape<4, 4, 4>(p, r, a, mol, has_rot, s);
	if (m * (6 * 4 * 4) <= cap) return launch_ardf_shape<4, 2, 2>(p, r, a, mol, has_rot, s);
	return launch_ardf_shape<2, 2, 2>(p, r, a, mol, has_rot, s);
}

}  // namespace ls1
