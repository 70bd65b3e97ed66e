// kernels_rdf.hip — radial distribution functions sampled on the device: the second traversal of the linked cells that the
// reference's RDF plugin runs after the forces (io/RDF.h:111-170, adapter/RDFCellProcessor.cpp:18-133).
//
//   * brick-tiled like k_force_ms_brick: one 256-thread workgroup per brick of BX x BY x BZ cells, the brick and its cutoff shell
//     staged ONCE into LDS in region-linear order (centre FP64 x y z, molecule id, component id; with site histograms the
//     quaternion too, normalised where the rotation is formed), one lane per owned molecule, full shell;
//   * a pair (i owned, j owned or halo image) is observed by the lane of i iff id_i < id_j and dd < rc^2, dd = dx*dx + dy*dy + dz*dz of
//     d = r_j - r_i (RDFCellProcessor.cpp:34,63): every unordered pair exactly once in the sum over all ranks, also across periodic
//     faces and rank boundaries, and never computed from two differently rounded sides (the reference's cell-index rule,
//     RDFCellProcessor.cpp:104-109, does the same for its half-shell traversal).  A molecule and its OWN periodic image share
//     the id and are not observed: boxes are at least two cutoffs long wherever a pair has one image inside the cutoff;
//   * bin = floor(sqrt(dd) / dr) with IEEE sqrt and division (RDF.h:138-146); dd > (bins dr)^2 and bin >= bins are dropped (the
//     reference would write behind its vector there);
//   * site histograms (RDF.h:111-133,152-170): every site m of i against every site n of j between ABSOLUTE site positions
//     r + R(q) d, sites ordered LJ centres, charges, dipoles, quadrupoles (FullMolecule.h:171-185); (i, j), (m, n) swapped when
//     ci > cj; ci == cj and m != n increments [m][n] and [n][m] (the reference's documented double count, RDF.cpp:558);
//   * counts go to a u32 histogram in LDS (atomicAdd on LDS), whose non-zero words are added to the global u64 histogram at the end:
//     integer atomics, so the result does not depend on the order and is bitwise reproducible.
//   * the walk over the neighbour rows only collects the hits (per-lane u16 lists in LDS, branch-free); sqrt, division, atomics and
//     the site loops run over the lists with every lane busy.
// LDS budget: RDF_LDS_WORDS u32 (8 KB) per workgroup for histograms, next to ~43 KB of staging and 16-24 KB of hit lists — 78 KB, two
// workgroups per CU.  The molecule histogram (pairs x bins words) lives there whenever it fits; the site histograms join it when
// BOTH fit, otherwise they go straight to global atomics (five 4-5-site components at 113 bins: the 1 695 molecule words stay in
// LDS, the site blocks do not fit).  A molecule histogram beyond the budget (e.g. fifteen pairs at more than 136 bins) goes to
// global atomics as well: slower, same counts.
#include "common.hpp"
#include "brick.hpp"

namespace ls1 {

constexpr int RTPB = 256;
constexpr int RDF_LDS_WORDS = 2048;

// position of site m (reference order: LJ centres, charges, dipoles, quadrupoles) of component c in the body frame
__device__ __forceinline__ V3 rdf_site_pos(const CompTable& ct, int c, int m) {
	if (m < ct.nlj[c]) return ld3(ct.ljpos, ct.olj[c] + m);
	m -= ct.nlj[c];
	if (m < ct.nc[c]) return ld3(ct.chpos, ct.oc[c] + m);
	m -= ct.nc[c];
	if (m < ct.nd[c]) return ld3(ct.dppos, ct.od[c] + m);
	m -= ct.nd[c];
	return ld3(ct.qppos, ct.oq[c] + m);
}

__device__ __forceinline__ Rot rdf_rot(double w, double x, double y, double z) {
	const double inv = 1. / sqrt(w * w + x * x + y * y + z * z);  // FullMolecule::setupSoACache normalises before rotating
	return rot_of(w * inv, x * inv, y * inv, z * inv);
}

template <int BX, int BY, int BZ, int CAPJ, int CAPL, bool SITE>
__global__ void __launch_bounds__(RTPB) k_rdf_brick(ForceParams P, RdfParams R, const CompTable* __restrict__ ctab, int has_rot, int nbx,
												   int nby, int nbz) {
	constexpr int HW = 1, NT = RTPB;
	constexpr int RX = BX + 2 * HW, RY = BY + 2 * HW, RZ = BZ + 2 * HW;
	constexpr int NRC = RX * RY * RZ;
	constexpr int NBC = BX * BY * BZ;
	constexpr int NW = 3, NROWS = 9;
	constexpr int QN = SITE ? CAPJ : 1;
	static_assert(NRC <= NT * 4 && NBC <= NT * 4, "region too large for the block scan");
	__shared__ double sx[CAPJ], sy[CAPJ], sz[CAPJ];
	__shared__ double sq0[QN], sq1[QN], sq2[QN], sq3[QN];  // quaternion as stored (normalised when the rotation is formed)
	__shared__ uint64_t sid[CAPJ];
	__shared__ uint8_t scid[CAPJ];
	__shared__ uint16_t lst[(CAPL + 1) * NT];  // slot-major per-lane hit lists; row CAPL = dummy target of misses / overflow
	__shared__ uint32_t cstart[NRC + 1];
	__shared__ uint32_t gbeg[NRC];
	__shared__ uint32_t bstart[NBC + 1];
	__shared__ uint32_t wsum[NT / 64];
	__shared__ uint32_t hist[RDF_LDS_WORDS];
	__shared__ uint32_t ncnt[MAXC];

	const int tid = threadIdx.x;
	const BrickSel bs = brick_select<HW, BX, BY, BZ>(P, nbx, nby, nbz);
	if (!bs.live) return;  // uniform per workgroup
	const int ex = bs.ex, ey = bs.ey, ez = bs.ez;
	const uint32_t mol_base = 0, site_base = R.mol_lds ? R.mol_words : 0u;
	const uint32_t lds_words = (R.mol_lds ? R.mol_words : 0u) + ((SITE && R.site_lds) ? R.site_words : 0u);  // <= RDF_LDS_WORDS (launch_rdf)
	for (uint32_t w = tid; w < lds_words; w += NT) hist[w] = 0u;
	if (tid < MAXC) ncnt[tid] = 0u;
	// ---- region cell table, brick cell prefix --------------------------------------------------------------------------
	brick_region_table<NT, HW, RX, RY, RZ>(P, bs, cstart, gbeg);
	__syncthreads();
	block_scan_lds<NT>(cstart, NRC, wsum);
	const uint32_t total = cstart[NRC];
	for (int c = tid; c < NBC; c += NT) {
		const int cx = c % BX, cy = (c / BX) % BY, cz = c / (BX * BY);
		uint32_t n = 0;
		if (cx < ex && cy < ey && cz < ez) {
			const int rcell = ((cz + HW) * RY + (cy + HW)) * RX + (cx + HW);
			n = cstart[rcell + 1] - cstart[rcell];
		}
		bstart[c] = n;
	}
	__syncthreads();
	block_scan_lds<NT>(bstart, NBC, wsum);
	const uint32_t n_i = bstart[NBC];
	const bool staged = total <= (uint32_t)CAPJ;
	const uint32_t n_real = P.cnt->n_real;
	// quaternion of slot g: a halo image takes it from its source molecule — between two builds of the neighbour lists only the
	// POSITIONS of the halo copies are refreshed (ls1hip_halo_refresh), the owned molecules' orientations are always current
	auto qslot = [&](uint32_t g) {
		if (g >= n_real) {
			const uint32_t s = R.hsrc[g - n_real];
			if (s != 0xffffffffu) return s;
		}
		return g;
	};
	if (staged) {
		for (uint32_t s = tid; s < total; s += NT) {
			int lo = 0, hi = NRC;
			while (hi - lo > 1) {
				const int mid = (lo + hi) >> 1;
				if (cstart[mid] <= s) lo = mid;
				else hi = mid;
			}
			const uint32_t g = gbeg[lo] + (s - cstart[lo]);
			sx[s] = P.x[g];
			sy[s] = P.y[g];
			sz[s] = P.z[g];
			sid[s] = R.id[g];
			scid[s] = (uint8_t)P.cid[g];
			if (SITE) {
				double w = 1., x = 0., y = 0., z = 0.;
				if (has_rot) {
					const uint32_t gq = qslot(g);
					w = P.q0[gq]; x = P.q1[gq]; y = P.q2[gq]; z = P.q3[gq];
				}
				sq0[s] = w; sq1[s] = x; sq2[s] = y; sq3[s] = z;
			}
		}
	}
	__syncthreads();

	const double rc2 = R.rc2, maxd2 = R.maxd2, dr = R.dr;
	const uint32_t bins = (uint32_t)R.bins;
	const int ncomp = R.ncomp;
	auto add_mol = [&](uint32_t w) {
		if (R.mol_lds) atomicAdd(&hist[mol_base + w], 1u);
		else atomicAdd(&R.g_mol[w], 1ull);
	};
	auto add_site = [&](uint32_t w) {
		if (R.site_lds) atomicAdd(&hist[site_base + w], 1u);
		else atomicAdd(&R.g_site[w], 1ull);
	};
	// one molecule pair inside the cutoff: RDF::observeRDF (RDF.h:111-133)
	auto observe = [&](double dd, int ci, V3 ri, const Rot& Ri, int cj, V3 rj, double jq0, double jq1, double jq2, double jq3) {
		const int ca = min(ci, cj), cb = max(ci, cj);
		const int pair = ca * ncomp - (ca * (ca - 1)) / 2 + (cb - ca);
		if (!(dd > maxd2)) {
			const double b = floor(sqrt(dd) / dr);
			if (b < (double)bins) add_mol((uint32_t)pair * bins + (uint32_t)b);
		}
		if (SITE) {
			const uint32_t off = R.site_off[pair];
			if (off == 0xffffffffu) return;
			const int ni = R.nsites[ci], nj = R.nsites[cj];
			const uint32_t nb = (uint32_t)R.nsites[cb];
			const Rot Rj = has_rot ? rdf_rot(jq0, jq1, jq2, jq3) : rot_of(1., 0., 0., 0.);
			for (int m = 0; m < ni; ++m) {
				const V3 pi = ri + rotate(Ri, rdf_site_pos(*ctab, ci, m));
				for (int n = 0; n < nj; ++n) {
					const V3 pj = rj + rotate(Rj, rdf_site_pos(*ctab, cj, n));
					const V3 d = pi - pj;  // SiteSiteDistanceAbs(dii, djj, ...)
					const double d2 = d.x * d.x + d.y * d.y + d.z * d.z;
					if (d2 > maxd2) continue;
					const double b = floor(sqrt(d2) / dr);
					if (!(b < (double)bins)) continue;
					const uint32_t mm = (uint32_t)(ci > cj ? n : m), nn = (uint32_t)(ci > cj ? m : n);
					add_site(off + (mm * nb + nn) * bins + (uint32_t)b);
					if (ci == cj && m != n) add_site(off + (nn * nb + mm) * bins + (uint32_t)b);
				}
			}
		}
	};

	uint16_t* const mylist = lst + tid;
	for (uint32_t base = 0; base < n_i; base += NT) {  // one pass unless the brick holds more than 256 molecules
		const uint32_t it = base + (uint32_t)tid;
		if (it >= n_i) continue;
		int lo = 0, hi = NBC;
		while (hi - lo > 1) {
			const int mid = (lo + hi) >> 1;
			if (bstart[mid] <= it) lo = mid;
			else hi = mid;
		}
		const int cx = lo % BX, cy = (lo / BX) % BY, cz = lo / (BX * BY);
		const int rcell = ((cz + HW) * RY + (cy + HW)) * RX + (cx + HW);
		const uint32_t k = it - bstart[lo];
		const uint32_t ii = cstart[rcell] + k;
		const uint32_t gi = gbeg[rcell] + k;
		const int rowbase = (cz * RY + cy) * RX + cx;  // first cell of row 0 of the neighbourhood
		if (staged) {
			const V3 ri = {sx[ii], sy[ii], sz[ii]};
			const int ci = (int)scid[ii];
			const uint64_t idi = sid[ii];
			const Rot Ri = (SITE && has_rot) ? rdf_rot(sq0[ii], sq1[ii], sq2[ii], sq3[ii]) : rot_of(1., 0., 0., 0.);
			atomicAdd(&ncnt[ci], 1u);
			// Phase 1 / phase 2 in windows of CAPL hits, as k_force_ms_brick: the walk over the 9 neighbour rows appends the hits
			// number [done, done + CAPL) branch-free to the per-lane list; the binning (IEEE sqrt and division, LDS atomics, the
			// site loops) then runs over the list with every lane busy.  About one candidate in twelve is a hit (inside r_c AND
			// the larger id), so binning inside the walk kept 63 lanes of a wave waiting for nearly every candidate.
			uint32_t done = 0, seen;
			do {
				seen = 0;
				uint32_t cnt = 0;
				for (int row = 0; row < NROWS; ++row) {
					const int r0 = rowbase + (row / NW) * (RY * RX) + (row % NW) * RX;
					const uint32_t jb = cstart[r0], je = cstart[r0 + NW];
#pragma unroll 4
					for (uint32_t j = jb; j < je; ++j) {
						const double dx = sx[j] - ri.x, dy = sy[j] - ri.y, dz = sz[j] - ri.z;
						const double dd = dx * dx + dy * dy + dz * dz;
						const bool hit = (dd < rc2) & (idi < sid[j]);
						const bool take = hit & (seen >= done) & (seen < done + (uint32_t)CAPL);
						mylist[(take ? seen - done : (uint32_t)CAPL) * NT] = (uint16_t)j;
						cnt += take ? 1u : 0u;
						seen += hit ? 1u : 0u;
					}
				}
				for (uint32_t s = 0; s < cnt; ++s) {
					const uint32_t j = mylist[s * NT];
					const V3 rj = {sx[j], sy[j], sz[j]};
					const double dx = rj.x - ri.x, dy = rj.y - ri.y, dz = rj.z - ri.z;
					const double dd = dx * dx + dy * dy + dz * dz;  // the same expression as in the walk: the same bits
					if (SITE) observe(dd, ci, ri, Ri, (int)scid[j], rj, sq0[j], sq1[j], sq2[j], sq3[j]);
					else observe(dd, ci, ri, Ri, (int)scid[j], rj, 1., 0., 0., 0.);
				}
				done += cnt;
			} while (seen > done);
		} else {
			// shell does not fit the staging area: same walk straight from global memory
			const V3 ri = {P.x[gi], P.y[gi], P.z[gi]};
			const int ci = P.cid[gi];
			const uint64_t idi = R.id[gi];
			Rot Ri = rot_of(1., 0., 0., 0.);
			if (SITE && has_rot) Ri = rdf_rot(P.q0[gi], P.q1[gi], P.q2[gi], P.q3[gi]);  // (gi is owned)
			atomicAdd(&ncnt[ci], 1u);
			for (int row = 0; row < NROWS; ++row) {
				const int r0 = rowbase + (row / NW) * (RY * RX) + (row % NW) * RX;
				for (int c = r0; c < r0 + NW; ++c) {
					const uint32_t g0 = gbeg[c], n = cstart[c + 1] - cstart[c];
					for (uint32_t j = g0; j < g0 + n; ++j) {
						const V3 rj = {P.x[j], P.y[j], P.z[j]};
						const double dx = rj.x - ri.x, dy = rj.y - ri.y, dz = rj.z - ri.z;
						const double dd = dx * dx + dy * dy + dz * dz;
						if (!((dd < rc2) & (idi < R.id[j]))) continue;
						if (SITE && has_rot) {
							const uint32_t jq = qslot(j);
							observe(dd, ci, ri, Ri, P.cid[j], rj, P.q0[jq], P.q1[jq], P.q2[jq], P.q3[jq]);
						} else {
							observe(dd, ci, ri, Ri, P.cid[j], rj, 1., 0., 0., 0.);
						}
					}
				}
			}
		}
	}
	__syncthreads();
	// ---- flush: non-zero words of the workgroup's histogram -> global u64 histogram ----------------------------------------------------
	for (uint32_t w = tid; w < lds_words; w += NT) {
		const uint32_t v = hist[w];
		if (v == 0u) continue;
		if (R.mol_lds && w < R.mol_words) atomicAdd(&R.g_mol[w], (unsigned long long)v);
		else atomicAdd(&R.g_site[w - site_base], (unsigned long long)v);
	}
	if (tid < ncomp && ncnt[tid]) atomicAdd(&R.g_n[tid], (unsigned long long)ncnt[tid]);
}

template <int BX, int BY, int BZ>
static bool launch_rdf_shape(ForceParams p, const RdfParams& r, bool site, bool has_rot, hipStream_t s) {
	const Grid& g = p.g;
	const int nbx = (g.box[0] + BX - 1) / BX, nby = (g.box[1] + BY - 1) / BY, nbz = (g.box[2] + BZ - 1) / BZ;
	const long nb = (long)nbx * nby * nbz;
	if (nb <= 0 || nb > 0x7ffffff0L) return false;
	p.which = 0;
	p.brick_list = nullptr;
	p.n_list = 0;
	p.inner_box = 0;
	p.did_mode = 0;
	p.brick_did = nullptr;
	const dim3 grid((uint32_t)(8 * ((nb + 7) / 8))), block(RTPB);  // multiple of 8: the XCD-aware order of brick_select
	if (site) hipLaunchKernelGGL((k_rdf_brick<BX, BY, BZ, 600, 31, true>), grid, block, 0, s, p, r, p.ct, has_rot ? 1 : 0, nbx, nby, nbz);
	else hipLaunchKernelGGL((k_rdf_brick<BX, BY, BZ, 1312, 47, false>), grid, block, 0, s, p, r, p.ct, 0, nbx, nby, nbz);
	return true;
}

// Staging costs 33 B per molecule (65 B with quaternions): 1312 / 600 molecules in 43 / 39 KB; a list row is 256 x 2 B (47 / 31 rows:
// a 1CLJ liquid at r_c 2.5 has ~27 hits per molecule, further hits take another walk).  The brick shape follows the mean cell
// occupancy as in launch_force_ms: the largest shape whose shell fits the staging area with 8 % headroom; a brick whose shell
// overflows all the same walks global memory (same arithmetic, same counts).
bool launch_rdf(const ForceParams& p, RdfParams r, bool has_rot, double mean_per_cell, hipStream_t s) {
	if (p.g.hw != 1 || p.ct == nullptr) return false;
	const bool site = r.site_words != 0;
	r.mol_lds = r.mol_words <= (uint32_t)RDF_LDS_WORDS;
	r.site_lds = site && r.mol_lds && r.mol_words + r.site_words <= (uint32_t)RDF_LDS_WORDS;
	const double m = mean_per_cell * 1.08, cap = site ? 600. : 1312.;
	if (m * (6 * 6 * 6) <= cap) return launch_rdf_shape<4, 4, 4>(p, r, site, has_rot, s);
	if (m * (6 * 4 * 4) <= cap) return launch_rdf_shape<4, 2, 2>(p, r, site, has_rot, s);
	return launch_rdf_shape<2, 2, 2>(p, r, site, has_rot, s);
}

}  // namespace ls1
