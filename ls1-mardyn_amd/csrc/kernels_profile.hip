// kernels_profile.hip — spatial profiles sampled on the device: the molecule loop of SpatialProfile::endStep
// (plugins/SpatialProfile.cpp:233-283) with the record() bodies of plugins/profiles/{Density,VelocityAbs,Velocity3d,DOF,Kinetic,
// Virial}Profile.h, as ONE pass over the owned molecules.
//
// A scatter-add of up to 10 words per molecule into a table that is often tiny (1 x 200 x 1) and sometimes large (1 x 256 x 256).
// Global float atomics run at one chip-wide byte rate and an order of magnitude below it when every adder meets on one row, so the
// pass never issues one atomic per molecule and quantity:
//   * persistent workgroups over contiguous chunks of the owned range (cell-sorted: the lanes of a wave hit the same few bins),
//     two neighbouring molecules per lane, 16-byte loads;
//   * the lanes of a row of 16 first merge RUNS of equal bin index (segmented scan with head flags, DPP row shifts: VALU only),
//     and only the last lane of a run adds;
//   * a table of at most PROF_LDS_WORDS words is accumulated in a private LDS copy per workgroup (ds_add_u64 / ds_add_f64) and
//     flushed once: non-zero words only, lanes on consecutive bins of one quantity array (contiguous 128-256 B per wave
//     instruction); a larger table takes one global atomic per run and quantity — after a per-workgroup LDS cache of
//     PROF_SLOTS bins (hashed by bin index, claimed by compare-and-swap on a tag) has absorbed the runs of the bins it holds: a
//     workgroup's contiguous chunk of cell-sorted molecules touches a few hundred bins at most, but neighbouring lanes
//     alternate between the 3 x 3 bins a cell column straddles, so runs alone stay short.  A run whose slot belongs to another
//     bin goes to the global table directly; the cache is flushed once, non-zero words only.
// Counts (u64) are exact.  The f64 sums depend on the arrival order of the adds and may differ in the last bits from run to run.
#include <algorithm>

#include "common.hpp"
#include "leapfrog_body.hpp"

namespace ls1 {

constexpr int PTPB = 256;                 // threads per workgroup
constexpr int PROF_PER_TRIP = 2 * PTPB;   // molecules a workgroup takes per trip
// LDS table budget per workgroup: 48 KB of the CU's 160 KB, i.e. three resident workgroups
constexpr uint32_t PROF_LDS_WORDS = 6144;
size_t profile_lds_words() { return PROF_LDS_WORDS; }
// the bin cache of the global path, inside the same LDS array: PROF_SLOTS slots of PROF_SLOT_WORDS words {n, dof, ekin, vabs, v3[3],
// vi3[3]}, then one u32 tag (the bin, PROF_EMPTY: free) per slot
constexpr uint32_t PROF_SLOTS = 512, PROF_SLOT_BITS = 9, PROF_SLOT_WORDS = 10, PROF_EMPTY = 0xffffffffu;
static_assert(PROF_SLOTS == 1u << PROF_SLOT_BITS && PROF_SLOTS * PROF_SLOT_WORDS + PROF_SLOTS / 2 <= PROF_LDS_WORDS, "cache fits the LDS array");

template <int CTRL>
__device__ __forceinline__ int prof_dpp_i(int old, int v) {
	return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false);  // lanes without a source keep `old`
}
template <int CTRL>
__device__ __forceinline__ double prof_dpp_d(double v) {
	const int lo = prof_dpp_i<CTRL>(0, __double2loint(v)), hi = prof_dpp_i<CTRL>(0, __double2hiint(v));
	return __hiloint2double(hi, lo);
}

// what one molecule adds: bin (-1: nothing), count, 3 + rotDOF, and the eight doubles {|v|, v[3], m v^2 + I w^2, Vi[3]}
struct ProfTerm {
	int key, n, dof;
	double v[8];
};
constexpr int PV_ABS = 0, PV_V3 = 1, PV_EKIN = 4, PV_VI = 5;

// One step of the segmented inclusive scan inside a row of 16 lanes (row_shr:S): a lane takes the partial sum of the lane S below
// it unless a run starts in between (head: OR of the head flags over the span already summed; lane 0 of a row is a head, so a
// lane without a source never adds).  Neighbouring runs may carry the same bin again (A B A): flags, not key comparisons at
// distance S, keep them apart.
template <int CTRL>
__device__ __forceinline__ void prof_seg_step(unsigned quant, int& head, ProfTerm& t) {
	const int hb = prof_dpp_i<CTRL>(1, head);
	const int tn = prof_dpp_i<CTRL>(0, t.n), td = prof_dpp_i<CTRL>(0, t.dof);
	double tv[8];
	if (quant & LS1HIP_PROF_VELOCITY) tv[PV_ABS] = prof_dpp_d<CTRL>(t.v[PV_ABS]);
	if (quant & LS1HIP_PROF_VELOCITY3D)
		for (int d = 0; d < 3; ++d) tv[PV_V3 + d] = prof_dpp_d<CTRL>(t.v[PV_V3 + d]);
	if (quant & LS1HIP_PROF_TEMPERATURE) tv[PV_EKIN] = prof_dpp_d<CTRL>(t.v[PV_EKIN]);
	if (quant & LS1HIP_PROF_VIRIAL)
		for (int d = 0; d < 3; ++d) tv[PV_VI + d] = prof_dpp_d<CTRL>(t.v[PV_VI + d]);
	if (!head) {
		t.n += tn;
		t.dof += td;
		if (quant & LS1HIP_PROF_VELOCITY) t.v[PV_ABS] += tv[PV_ABS];
		if (quant & LS1HIP_PROF_VELOCITY3D)
			for (int d = 0; d < 3; ++d) t.v[PV_V3 + d] += tv[PV_V3 + d];
		if (quant & LS1HIP_PROF_TEMPERATURE) t.v[PV_EKIN] += tv[PV_EKIN];
		if (quant & LS1HIP_PROF_VIRIAL)
			for (int d = 0; d < 3; ++d) t.v[PV_VI + d] += tv[PV_VI + d];
	}
	head |= hb;
}

template <bool LDS>
__device__ __forceinline__ void prof_add_u64(unsigned long long* tab, uint32_t w, unsigned long long v) {
	atomicAdd(&tab[w], v);  // LDS: ds_add_u64; global: global_atomic_add_x2
}
template <bool LDS>
__device__ __forceinline__ void prof_add_f64(unsigned long long* tab, uint32_t w, double v) {
	unsafeAtomicAdd(reinterpret_cast<double*>(tab) + w, v);  // LDS: ds_add_f64; global: global_atomic_add_f64 (no CAS loop)
}

// global word of slot word k of bin b (the table layout of ProfParams)
__device__ __forceinline__ uint32_t prof_slot_word(const ProfParams& P, uint32_t b, uint32_t k) {
	if (k == 0) return b;
	if (k == 1) return P.off_dof + b;
	if (k == 2) return P.off_ekin + b;
	if (k == 3) return P.off_vabs + b;
	if (k < 7) return P.off_v3 + 3u * b + (k - 4);
	return P.off_vi + 3u * b + (k - 7);
}

// the whole wave calls this (uniform control flow); lds: the workgroup's LDS table (LDS) or its bin cache
template <bool LDS>
__device__ __forceinline__ void prof_emit(const ProfParams& P, unsigned long long* lds, ProfTerm t) {
	const unsigned quant = P.quant;
	int head = prof_dpp_i<0x111>(-2, t.key) != t.key ? 1 : 0;        // row_shr:1 — the lane below starts another run / row start
	const bool last = prof_dpp_i<0x101>(-2, t.key) != t.key;          // row_shl:1 — the lane above continues the run?
	prof_seg_step<0x111>(quant, head, t);
	prof_seg_step<0x112>(quant, head, t);
	prof_seg_step<0x114>(quant, head, t);
	prof_seg_step<0x118>(quant, head, t);
	if (!last || t.key < 0) return;
	const uint32_t b = (uint32_t)t.key;
	if (!LDS) {
		const uint32_t slot = (b * 0x9E3779B1u) >> (32 - PROF_SLOT_BITS);
		uint32_t* const tags = reinterpret_cast<uint32_t*>(lds + PROF_SLOTS * PROF_SLOT_WORDS);
		const uint32_t owner = atomicCAS(&tags[slot], PROF_EMPTY, b);
		if (owner == PROF_EMPTY || owner == b) {
			unsigned long long* const sw = lds + slot * PROF_SLOT_WORDS;
			prof_add_u64<true>(sw, 0, (unsigned long long)t.n);
			if (quant & LS1HIP_PROF_TEMPERATURE) {
				prof_add_u64<true>(sw, 1, (unsigned long long)t.dof);
				prof_add_f64<true>(sw, 2, t.v[PV_EKIN]);
			}
			if (quant & LS1HIP_PROF_VELOCITY) prof_add_f64<true>(sw, 3, t.v[PV_ABS]);
			if (quant & LS1HIP_PROF_VELOCITY3D)
				for (int d = 0; d < 3; ++d) prof_add_f64<true>(sw, 4 + d, t.v[PV_V3 + d]);
			if (quant & LS1HIP_PROF_VIRIAL)
				for (int d = 0; d < 3; ++d) prof_add_f64<true>(sw, 7 + d, t.v[PV_VI + d]);
			return;
		}
	}
	unsigned long long* const tab = LDS ? lds : P.tab;  // (the slot belongs to another bin: straight to the global table)
	prof_add_u64<LDS>(tab, b, (unsigned long long)t.n);
	if (quant & LS1HIP_PROF_TEMPERATURE) {
		prof_add_u64<LDS>(tab, P.off_dof + b, (unsigned long long)t.dof);
		prof_add_f64<LDS>(tab, P.off_ekin + b, t.v[PV_EKIN]);
	}
	if (quant & LS1HIP_PROF_VELOCITY) prof_add_f64<LDS>(tab, P.off_vabs + b, t.v[PV_ABS]);
	if (quant & LS1HIP_PROF_VELOCITY3D)
		for (int d = 0; d < 3; ++d) prof_add_f64<LDS>(tab, P.off_v3 + 3u * b + d, t.v[PV_V3 + d]);
	if (quant & LS1HIP_PROF_VIRIAL)
		for (int d = 0; d < 3; ++d) prof_add_f64<LDS>(tab, P.off_vi + 3u * b + d, t.v[PV_VI + d]);
}

// GLOBAL coordinate wrapped into [0, L): between two builds of the neighbour lists a molecule may sit up to skin / 2 outside the
// box (the rule and the rounding clamps of ls1hip_download_state and of the re-binning pass, DomainDecompBase.cpp:206-219)
__device__ __forceinline__ double prof_wrap(double x, double len) {
	if (x < 0.) {
		x += len;
		if (x >= len) x = nextafter(len, 0.);
	} else if (x >= len) {
		x -= len;
		if (x <= 0.) x = 0.;
	}
	return x;
}
__device__ __forceinline__ int prof_unit(double u, uint32_t n) {
	int i = (int)floor(u);
	if (i < 0) i = 0;
	if (i > (int)n - 1) i = (int)n - 1;  // a product that rounds to n at the upper face
	return i;
}

// bin of one molecule: SpatialProfile::getCartesianUID / getCylUID (SpatialProfile.cpp:339-410), operation for operation
__device__ __forceinline__ int prof_bin(const ProfParams& P, double x, double y, double z) {
	x = prof_wrap(x, P.len[0]);
	y = prof_wrap(y, P.len[1]);
	z = prof_wrap(z, P.len[2]);
	if (P.mode == LS1HIP_PROF_CARTESIAN) {
		const int xun = prof_unit(x * P.inv[0], P.units[0]), yun = prof_unit(y * P.inv[1], P.units[1]),
				  zun = prof_unit(z * P.inv[2], P.units[2]);
		return (int)((uint32_t)xun * P.units[1] * P.units[2] + (uint32_t)yun * P.units[2] + (uint32_t)zun);
	}
	const double xc = x - P.centre[0], yc = y - P.centre[1], zc = z - P.centre[2];
	const double R2 = xc * xc + zc * zc;
	double phi = atan2(zc, xc);
	if (phi < 0.0) phi = phi + 2.0 * M_PI;
	const double rU = floor(R2 * P.inv[0]);
	if (!(rU < (double)P.units[0])) return -1;  // rUn >= nR: outside the cylinder (compared before the conversion to int)
	const int rUn = (int)rU;
	const int hUn = prof_unit(yc * P.inv[1], P.units[1]), phiUn = prof_unit(phi * P.inv[2], P.units[2]);
	return (int)((uint32_t)hUn * P.units[0] * P.units[2] + (uint32_t)(rUn < 0 ? 0 : rUn) * P.units[2] + (uint32_t)phiUn);
}

template <bool HAS_ROT>
__device__ __forceinline__ void prof_term(const ProfParams& P, uint32_t p, double x, double y, double z, int c, double bt, double br,
										   ProfTerm& t) {
	t.key = -1;
	t.n = t.dof = 0;
	for (int k = 0; k < 8; ++k) t.v[k] = 0.;
	if (P.comp >= 0 && c != P.comp) return;
	t.key = prof_bin(P, x, y, z);
	if (t.key < 0) return;
	t.n = 1;
	const unsigned quant = P.quant;
	if (!(quant & (LS1HIP_PROF_VELOCITY | LS1HIP_PROF_VELOCITY3D | LS1HIP_PROF_TEMPERATURE | LS1HIP_PROF_VIRIAL))) return;
	if (quant & (LS1HIP_PROF_VELOCITY | LS1HIP_PROF_VELOCITY3D | LS1HIP_PROF_TEMPERATURE)) {
		// (the thermostat's scaling as k_scale does it: v * beta_trans, D * beta_rot; factors 1 without it)
		const double vx = P.vx[p] * bt, vy = P.vy[p] * bt, vz = P.vz[p] * bt;
		if (quant & LS1HIP_PROF_VELOCITY) {
			double absV = 0.0;
			absV += vx * vx;
			absV += vy * vy;
			absV += vz * vz;
			t.v[PV_ABS] = sqrt(absV);
		}
		if (quant & LS1HIP_PROF_VELOCITY3D) {
			t.v[PV_V3] = vx; t.v[PV_V3 + 1] = vy; t.v[PV_V3 + 2] = vz;
		}
		if (quant & LS1HIP_PROF_TEMPERATURE) {
			double mv2, Iw2;
			if (HAS_ROT)
				kinetic_terms<true>(P.ct->mass[c], P.ct->I[c], P.ct->invI[c], vx, vy, vz, P.q0[p], P.q1[p], P.q2[p], P.q3[p],
									V3{P.Dx[p] * br, P.Dy[p] * br, P.Dz[p] * br}, mv2, Iw2);
			else
				kinetic_terms<false>(P.ct->mass[c], P.ct->I[c], P.ct->invI[c], vx, vy, vz, 1., 0., 0., 0., V3{0., 0., 0.}, mv2, Iw2);
			t.v[PV_EKIN] = mv2 + Iw2;
			t.dof = 3 + P.ct->rotdof[c];
		}
	}
	if (quant & LS1HIP_PROF_VIRIAL) {
		t.v[PV_VI] = P.Vix[p]; t.v[PV_VI + 1] = P.Viy[p]; t.v[PV_VI + 2] = P.Viz[p];
	}
}

template <bool HAS_ROT, bool LDS>
__global__ void __launch_bounds__(PTPB) k_profile(ProfParams P) {
	__shared__ unsigned long long lds_tab[PROF_LDS_WORDS];
	unsigned long long* const tab = lds_tab;
	if (LDS) {
		for (uint32_t w = threadIdx.x; w < P.words; w += PTPB) lds_tab[w] = 0ull;
	} else {
		for (uint32_t w = threadIdx.x; w < PROF_SLOTS * PROF_SLOT_WORDS; w += PTPB) lds_tab[w] = 0ull;
		uint32_t* const tags = reinterpret_cast<uint32_t*>(lds_tab + PROF_SLOTS * PROF_SLOT_WORDS);
		for (uint32_t w = threadIdx.x; w < PROF_SLOTS; w += PTPB) tags[w] = PROF_EMPTY;
	}
	__syncthreads();
	const uint32_t n = P.cnt->n_real;
	// contiguous chunk of whole trips per workgroup (uniform trip count inside a workgroup: every lane takes part in the scans)
	const uint32_t trips = (n + PROF_PER_TRIP - 1) / PROF_PER_TRIP;
	const uint32_t per = (trips + gridDim.x - 1) / gridDim.x;
	const uint32_t t0 = blockIdx.x * per, t1 = min(t0 + per, trips);
	double bt = 1., br = 1.;
	if (P.scale) {
		bt = P.cnt->beta[0];
		br = P.cnt->beta[1];
	}
	const bool need_cid = P.ncomp > 1;
	for (uint32_t t = t0; t < t1; ++t) {
		const uint32_t p = t * PROF_PER_TRIP + 2u * threadIdx.x;  // even: the 16-byte loads are aligned
		double2 X = {0., 0.}, Y = {0., 0.}, Z = {0., 0.};
		int c0 = 0, c1 = 0;
		if (p + 1 < n) {
			X = *reinterpret_cast<const double2*>(P.x + p);
			Y = *reinterpret_cast<const double2*>(P.y + p);
			Z = *reinterpret_cast<const double2*>(P.z + p);
			if (need_cid) {
				const int2 cc = *reinterpret_cast<const int2*>(P.cid + p);
				c0 = cc.x;
				c1 = cc.y;
			}
		} else if (p < n) {
			X.x = P.x[p]; Y.x = P.y[p]; Z.x = P.z[p];
			if (need_cid) c0 = P.cid[p];
		}
		ProfTerm a, b;
		a.key = b.key = -1;
		a.n = a.dof = b.n = b.dof = 0;
		for (int k = 0; k < 8; ++k) a.v[k] = b.v[k] = 0.;
		if (p < n) prof_term<HAS_ROT>(P, p, X.x, Y.x, Z.x, c0, bt, br, a);
		if (p + 1 < n) prof_term<HAS_ROT>(P, p + 1, X.y, Y.y, Z.y, c1, bt, br, b);
		if (b.key >= 0 && b.key == a.key) {  // the lane's two molecules share a bin: one term
			a.n += b.n;
			a.dof += b.dof;
			for (int k = 0; k < 8; ++k) a.v[k] += b.v[k];
			b.key = -1;
		}
		prof_emit<LDS>(P, tab, a);
		prof_emit<LDS>(P, tab, b);
	}
	if (LDS) {
		__syncthreads();
		// one flush: non-zero words only; lanes on consecutive words of one quantity array
		for (uint32_t w = threadIdx.x; w < P.words; w += PTPB) {
			const unsigned long long v = lds_tab[w];
			if (v == 0ull) continue;
			if (w < P.u64_words) atomicAdd(&P.tab[w], v);
			else unsafeAtomicAdd(reinterpret_cast<double*>(P.tab) + w, __longlong_as_double((long long)v));
		}
	} else {
		__syncthreads();
		// the bin cache: lanes on consecutive slots of one quantity, non-zero words of claimed slots only
		const uint32_t* const tags = reinterpret_cast<const uint32_t*>(lds_tab + PROF_SLOTS * PROF_SLOT_WORDS);
		for (uint32_t i = threadIdx.x; i < PROF_SLOTS * PROF_SLOT_WORDS; i += PTPB) {
			const uint32_t k = i >> PROF_SLOT_BITS, slot = i & (PROF_SLOTS - 1u);
			const uint32_t b = tags[slot];
			const unsigned long long v = lds_tab[slot * PROF_SLOT_WORDS + k];
			if (b == PROF_EMPTY || v == 0ull) continue;
			const uint32_t w = prof_slot_word(P, b, k);
			if (k < 2) atomicAdd(&P.tab[w], v);
			else unsafeAtomicAdd(reinterpret_cast<double*>(P.tab) + w, __longlong_as_double((long long)v));
		}
	}
}

void launch_profile(const ProfParams& p, bool has_rot, uint32_t n_cap, hipStream_t s) {
	if (n_cap == 0) return;
	const uint32_t trips = (n_cap + PROF_PER_TRIP - 1) / PROF_PER_TRIP;
	static int ncu = 0;
	if (!ncu) {
		int dev = 0;
		hipDeviceProp_t prop;
		if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
		if (ncu <= 0) ncu = 256;
	}
	const bool lds = p.words <= PROF_LDS_WORDS;
	// persistent: at most three workgroups per CU (the LDS budget); a workgroup with an LDS table takes at least four trips
	// so that its flush is shared by 2 048 molecules
	uint32_t nb = std::min<uint32_t>(trips, 3u * (uint32_t)ncu);
	if (lds) nb = std::min<uint32_t>(nb, std::max<uint32_t>(1u, trips / 4u));
	if (has_rot) {
		if (lds) hipLaunchKernelGGL((k_profile<true, true>), dim3(nb), dim3(PTPB), 0, s, p);
		else hipLaunchKernelGGL((k_profile<true, false>), dim3(nb), dim3(PTPB), 0, s, p);
	} else {
		if (lds) hipLaunchKernelGGL((k_profile<false, true>), dim3(nb), dim3(PTPB), 0, s, p);
		else hipLaunchKernelGGL((k_profile<false, false>), dim3(nb), dim3(PTPB), 0, s, p);
	}
}

}  // namespace ls1
