// kernels_tempcontrol.hip — region-wise temperature control on the device: the reference's TemperatureControl with the method
// VelocityScaling (thermostats/TemperatureControl.{h,cpp}), i.e. per control region a stack of slabs along y, each slab with its own
// kinetic sums and its own scaling factors.
//
//   k_tc_measure     ControlRegionT::MeasureKineticEnergy (TemperatureControl.cpp:308-362) for every owned molecule and region
//   k_tc_betas       ControlRegionT::CalcGlobalValues, the part after the all-reduce (:279-305)
//   k_tc_apply       ControlRegionT::ControlTemperature (:364-409) for every owned molecule and region, regions in their order
//   k_tc_kick_drift  the same scaling followed by the arithmetic of k_kick_drift (kernels_integrate.hip) in one pass
//
// The measure sweep is a scatter-add of four words per molecule and region into a table that is tiny (20 slabs is the usual
// setting), so it never issues one global atomic per molecule:
//   * persistent workgroups over contiguous chunks of the owned range, one lane per molecule; the range is cell-sorted, so the lanes
//     of a row of 16 mostly share a slab: per region, RUNS of equal slab index are merged with a segmented scan over DPP row shifts
//     (VALU only), and only the last lane of a run adds;
//   * the runs go to a per-workgroup LDS table [slab of any region]{n, rotDOF, ekinRot, ekinTrans} (ds_add_u64 / ds_add_f64), which is
//     flushed once, non-zero words only; with more than TC_LDS_SLABS slabs in all regions together the runs go to the global
//     table directly (one global atomic per run and word);
//   * the region descriptors are kernel arguments: the component filter and the direction flags are wave-uniform and cost
//     selects, no divergent branch.
// The apply passes read two factors per slab; a workgroup stages them in LDS when all regions together have at most
// TC_APPLY_LDS_SLABS slabs (a workgroup of 256 molecules should not read more table than molecule data), else it reads global memory.
//
// Counts (u64) are exact.  The f64 slab sums depend on the arrival order of the adds and may differ in the last bits from run to
// run; everything derived from one set of sums (betas, factors, the scaling) is deterministic.
#include <algorithm>

#include "common.hpp"
#include "leapfrog_body.hpp"

namespace ls1 {

constexpr int TTPB = 256;  // threads per workgroup
constexpr uint32_t TC_LDS_SLABS = 1024;       // 32 KB of sums per workgroup of the measure sweep
constexpr uint32_t TC_APPLY_LDS_SLABS = 256;  // 4 KB of factors per workgroup of the apply passes
size_t tempcontrol_lds_slabs() { return TC_LDS_SLABS; }
size_t tempcontrol_apply_lds_slabs() { return TC_APPLY_LDS_SLABS; }

template <int CTRL>
__device__ __forceinline__ int tc_dpp_i(int old, int v) {
	return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false);  // lanes without a source keep `old`
}
template <int CTRL>
__device__ __forceinline__ double tc_dpp_d(double v) {
	const int lo = tc_dpp_i<CTRL>(0, __double2loint(v)), hi = tc_dpp_i<CTRL>(0, __double2hiint(v));
	return __hiloint2double(hi, lo);
}

// what one molecule adds to one region: slab in the tables (-1: nothing), count, rotational DOF, the two kinetic terms
struct TcTerm {
	int key, n, dof;
	double et, er;
};

// One step of the segmented inclusive scan inside a row of 16 lanes (row_shr:S): a lane takes the partial sum of the lane S below
// it unless a run starts in between (head: OR of the head flags over the span already summed; lane 0 of a row is a head, so a
// lane without a source never adds).
template <int CTRL>
__device__ __forceinline__ void tc_seg_step(int& head, TcTerm& t) {
	const int hb = tc_dpp_i<CTRL>(1, head);
	const int tn = tc_dpp_i<CTRL>(0, t.n), td = tc_dpp_i<CTRL>(0, t.dof);
	const double tet = tc_dpp_d<CTRL>(t.et), ter = tc_dpp_d<CTRL>(t.er);
	if (!head) {
		t.n += tn;
		t.dof += td;
		t.et += tet;
		t.er += ter;
	}
	head |= hb;
}

// the whole wave calls this (uniform control flow); tab: the workgroup's LDS table or the global one, [slab][4]
template <bool HAS_ROT>
__device__ __forceinline__ void tc_emit(unsigned long long* tab, TcTerm t) {
	int head = tc_dpp_i<0x111>(-2, t.key) != t.key ? 1 : 0;  // row_shr:1 — the lane below starts another run / row start
	const bool last = tc_dpp_i<0x101>(-2, t.key) != t.key;    // row_shl:1 — the lane above continues the run?
	tc_seg_step<0x111>(head, t);
	tc_seg_step<0x112>(head, t);
	tc_seg_step<0x114>(head, t);
	tc_seg_step<0x118>(head, t);
	if (!last || t.key < 0) return;
	unsigned long long* const e = tab + 4u * (uint32_t)t.key;
	atomicAdd(e + TC_N, (unsigned long long)t.n);  // LDS: ds_add_u64; global: global_atomic_add_x2
	unsafeAtomicAdd(reinterpret_cast<double*>(e) + TC_EKIN_TRANS, t.et);  // LDS: ds_add_f64; global: global_atomic_add_f64 (no CAS loop)
	if (HAS_ROT) {
		atomicAdd(e + TC_ROTDOF, (unsigned long long)t.dof);
		unsafeAtomicAdd(reinterpret_cast<double*>(e) + TC_EKIN_ROT, t.er);
	}
}

// GLOBAL coordinate wrapped into [0, L): between two builds of the neighbour lists a molecule may sit up to skin / 2 outside the
// box (the rule and the rounding clamps of ls1hip_download_state and of the profile pass, DomainDecompBase.cpp:206-219)
__device__ __forceinline__ double tc_wrap(double x, double len) {
	if (x < 0.) {
		x += len;
		if (x >= len) x = nextafter(len, 0.);
	} else if (x >= len) {
		x -= len;
		if (x <= 0.) x = 0.;
	}
	return x;
}

// slab of a molecule in region R, index into the tables; -1: the molecule takes no part (TemperatureControl.cpp:310-333, 365-390)
__device__ __forceinline__ int tc_slab(const TcRegion& R, int c, double x, double y, double z) {
	bool in = R.comp == 0 || c + 1 == R.comp;
	in = in && !(x <= R.lc[0] || x >= R.uc[0]) && !(y <= R.lc[1] || y >= R.uc[1]) && !(z <= R.lc[2] || z >= R.uc[2]);
	const double dPosRelative = y - R.lc[1];
	const double f = floor(dPosRelative / R.width);
	// (unsigned int) of the reference: a negative value becomes a large one; compared as doubles before the conversion
	in = in && f >= 0. && f <= (double)(R.slabs - 1u);
	return in ? (int)(R.off + (uint32_t)f) : -1;
}

template <bool HAS_ROT, bool LDS>
__global__ void __launch_bounds__(TTPB) k_tc_measure(TcParams P) {
	__shared__ unsigned long long lds_tab[LDS ? TC_LDS_SLABS * 4 : 1];
	const uint32_t words = 4u * P.total;
	if (LDS) {
		for (uint32_t w = threadIdx.x; w < words; w += TTPB) lds_tab[w] = 0ull;
		__syncthreads();
	}
	unsigned long long* const tab = LDS ? lds_tab : P.sums;
	const uint32_t n = P.cnt->n_real;
	// contiguous chunk of whole trips per workgroup (uniform trip count inside a workgroup: every lane takes part in the scans)
	const uint32_t trips = (n + TTPB - 1) / TTPB;
	const uint32_t per = (trips + gridDim.x - 1) / gridDim.x;
	const uint32_t t0 = blockIdx.x * per, t1 = min(t0 + per, trips);
	for (uint32_t t = t0; t < t1; ++t) {
		const uint32_t p = t * TTPB + threadIdx.x;
		const bool live = p < n;
		double x = 0., y = 0., z = 0., vx = 0., vy = 0., vz = 0., mass = 0., Iw2 = 0.;
		int c = 0, rdof = 0;
		if (live) {
			x = tc_wrap(P.x[p], P.len[0]);
			y = tc_wrap(P.y[p], P.len[1]);
			z = tc_wrap(P.z[p], P.len[2]);
			vx = P.vx[p]; vy = P.vy[p]; vz = P.vz[p];
			c = P.ncomp > 1 ? P.cid[p] : 0;
			mass = P.ct->mass[c];
			if (HAS_ROT) {
				// calculate_mv2_Iw2 (TemperatureControl.cpp:354): the term of leapfrog_body.hpp
				double mv2;
				kinetic_terms<true>(mass, P.ct->I[c], P.ct->invI[c], vx, vy, vz, P.q0[p], P.q1[p], P.q2[p], P.q3[p], V3{P.Dx[p], P.Dy[p], P.Dz[p]},
									mv2, Iw2);
				rdof = P.ct->rotdof[c];
			}
		}
		for (int r = 0; r < P.nreg; ++r) {  // (uniform)
			const TcRegion& R = P.reg[r];
			TcTerm a;
			a.key = live ? tc_slab(R, c, x, y, z) : -1;
			if (__ballot(a.key >= 0) == 0ull) continue;  // (uniform: no lane of the wave is inside this region)
			const bool in = a.key >= 0;
			// Accumulator::CalcKineticEnergyContribution (TemperatureControl.h:218-225): the flags are uniform selects
			const double ax = R.dir[0] ? vx : 0.0, ay = R.dir[1] ? vy : 0.0, az = R.dir[2] ? vz : 0.0;
			a.n = in ? 1 : 0;
			a.dof = in ? rdof : 0;
			a.et = in ? mass * (ax * ax + ay * ay + az * az) : 0.;
			a.er = in ? Iw2 : 0.;
			tc_emit<HAS_ROT>(tab, a);
		}
	}
	if (LDS) {
		__syncthreads();
		// one flush: non-zero words only
		for (uint32_t w = threadIdx.x; w < words; w += TTPB) {
			const unsigned long long v = lds_tab[w];
			if (v == 0ull) continue;
			if ((w & 3u) < 2u) atomicAdd(&P.sums[w], v);
			else unsafeAtomicAdd(reinterpret_cast<double*>(P.sums) + w, __longlong_as_double((long long)v));
		}
	}
}

void launch_tc_measure(const TcParams& p, bool has_rot, uint32_t n_cap, hipStream_t s) {
	if (n_cap == 0 || p.nreg == 0) return;
	const uint32_t trips = (n_cap + TTPB - 1) / TTPB;
	static int ncu = 0;
	if (!ncu) {
		int dev = 0;
		hipDeviceProp_t prop;
		if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
		if (ncu <= 0) ncu = 256;
	}
	const bool lds = p.total <= TC_LDS_SLABS;
	// persistent: at most four workgroups per CU (the LDS budget); a workgroup with an LDS table takes at least eight trips so that
	// its flush is shared by 2 048 molecules
	uint32_t nb = std::min<uint32_t>(trips, 4u * (uint32_t)ncu);
	if (lds) nb = std::min<uint32_t>(nb, std::max<uint32_t>(1u, trips / 8u));
	if (has_rot) {
		if (lds) hipLaunchKernelGGL((k_tc_measure<true, true>), dim3(nb), dim3(TTPB), 0, s, p);
		else hipLaunchKernelGGL((k_tc_measure<true, false>), dim3(nb), dim3(TTPB), 0, s, p);
	} else {
		if (lds) hipLaunchKernelGGL((k_tc_measure<false, true>), dim3(nb), dim3(TTPB), 0, s, p);
		else hipLaunchKernelGGL((k_tc_measure<false, false>), dim3(nb), dim3(TTPB), 0, s, p);
	}
}

// sums = 0, factors = 1 (count 0: the slab is skipped), accumulators = 0 — the state of a region before its first measurement
__global__ void __launch_bounds__(TTPB) k_tc_init(TcParams P) {
	const uint32_t i = blockIdx.x * TTPB + threadIdx.x;
	if (i < 4u * P.total) {
		P.sums[i] = 0ull;
		P.last[i] = 0ull;
		P.fac[i] = 1.;
	}
	if (i < 2u * (uint32_t)P.nreg) P.acc[i] = 0.;
}
void launch_tc_init(const TcParams& p, hipStream_t s) {
	if (p.nreg == 0) return;
	hipLaunchKernelGGL(k_tc_init, dim3((4u * p.total + TTPB - 1) / TTPB), dim3(TTPB), 0, s, p);
}
__global__ void k_tc_clear_acc(TcParams P, int region) {
	if (threadIdx.x < 2) P.acc[2 * region + threadIdx.x] = 0.;
}
void launch_tc_clear_acc(const TcParams& p, int region, hipStream_t s) {
	hipLaunchKernelGGL(k_tc_clear_acc, dim3(1), dim3(64), 0, s, p, region);
}

// One workgroup per region over its slabs: betas and factors of every slab (TemperatureControl.cpp:283-301, 396-397), the sums over
// the slabs added to the region's accumulators (:303-304; folded in a fixed order, not the slab order of the reference), the sums
// kept as those of the last measurement and zeroed for the next one.
__global__ void __launch_bounds__(TTPB) k_tc_betas(TcParams P) {
	const TcRegion& R = P.reg[blockIdx.x];
	double sbt = 0., sbr = 0.;
	for (uint32_t s = threadIdx.x; s < R.slabs; s += TTPB) {
		const uint32_t e = 4u * (R.off + s);
		const unsigned long long n = P.sums[e + TC_N], dof = P.sums[e + TC_ROTDOF];
		const double ekr = __longlong_as_double((long long)P.sums[e + TC_EKIN_ROT]), ekt = __longlong_as_double((long long)P.sums[e + TC_EKIN_TRANS]);
		double bt = 1., br = 1.;
		if (n >= 1) bt = pow(R.ndir * n * R.target_T / ekt, R.exponent);
		if (dof >= 1) br = pow(dof * R.target_T / ekr, R.exponent);
		P.fac[e + TC_BETA_TRANS] = bt;
		P.fac[e + TC_BETA_ROT] = br;
		P.fac[e + TC_VCORR] = 2. - 1. / bt;  // (a slab with n < 1 has both betas 1: factors 1, the skip of :393)
		P.fac[e + TC_DCORR] = 2. - 1. / br;
		for (int k = 0; k < 4; ++k) {
			P.last[e + k] = P.sums[e + k];
			P.sums[e + k] = 0ull;
		}
		sbt += bt;
		sbr += br;
	}
	__shared__ double red[TTPB / 64][2];
	sbt = wave_fold_sum(sbt);
	sbr = wave_fold_sum(sbr);
	if ((threadIdx.x & 63) == 0) {
		red[threadIdx.x >> 6][0] = sbt;
		red[threadIdx.x >> 6][1] = sbr;
	}
	__syncthreads();
	if (threadIdx.x < 2) {
		double v = 0.;
		for (int i = 0; i < TTPB / 64; ++i) v += red[i][threadIdx.x];
		P.acc[2 * blockIdx.x + threadIdx.x] += v;
	}
}
void launch_tc_betas(const TcParams& p, hipStream_t s) {
	if (p.nreg == 0) return;
	hipLaunchKernelGGL(k_tc_betas, dim3(p.nreg), dim3(TTPB), 0, s, p);
}

// the factors of all regions' slabs {vcorr, Dcorr}: staged in LDS by the workgroup or read from global memory
template <bool LDS>
struct TcFactors {
	const double* g;
	double (*l)[2];
	__device__ __forceinline__ double v(int key) const { return LDS ? l[key][0] : g[4 * key + TC_VCORR]; }
	__device__ __forceinline__ double d(int key) const { return LDS ? l[key][1] : g[4 * key + TC_DCORR]; }
};
template <bool LDS>
__device__ __forceinline__ void tc_stage(const TcParams& P, double (*l)[2]) {
	if (!LDS) return;
	for (uint32_t s = threadIdx.x; s < P.total; s += TTPB) {
		l[s][0] = P.fac[4u * s + TC_VCORR];
		l[s][1] = P.fac[4u * s + TC_DCORR];
	}
	__syncthreads();
}

// ControlTemperature of every region, in their order, on the values of one molecule: the masked velocity components times vcorr
// (Accumulator::ScaleVelocityComponents), all of D times Dcorr (scale_D).  A factor of exactly 1 where the reference does not
// multiply: the bits stay.
template <bool HAS_ROT, bool LDS>
__device__ __forceinline__ void tc_scale(const TcParams& P, const TcFactors<LDS>& F, int c, double x, double y, double z, double& vx, double& vy,
										 double& vz, V3& D) {
	x = tc_wrap(x, P.len[0]);
	y = tc_wrap(y, P.len[1]);
	z = tc_wrap(z, P.len[2]);
	for (int r = 0; r < P.nreg; ++r) {  // (uniform)
		const TcRegion& R = P.reg[r];
		const int key = tc_slab(R, c, x, y, z);
		const double vcorr = key >= 0 ? F.v(key) : 1., Dcorr = key >= 0 ? F.d(key) : 1.;
		vx = vx * (R.dir[0] ? vcorr : 1.);
		vy = vy * (R.dir[1] ? vcorr : 1.);
		vz = vz * (R.dir[2] ? vcorr : 1.);
		if (HAS_ROT) D = {D.x * Dcorr, D.y * Dcorr, D.z * Dcorr};
	}
}

template <bool HAS_ROT, bool LDS>
__global__ void __launch_bounds__(TTPB) k_tc_apply(TcParams P) {
	__shared__ double lfac[LDS ? TC_APPLY_LDS_SLABS : 1][2];
	tc_stage<LDS>(P, lfac);
	const TcFactors<LDS> F = {P.fac, lfac};
	const uint32_t p = blockIdx.x * TTPB + threadIdx.x;
	if (p >= P.cnt->n_real) return;
	const int c = P.ncomp > 1 ? P.cid[p] : 0;
	double vx = P.vx[p], vy = P.vy[p], vz = P.vz[p];
	V3 D = {0., 0., 0.};
	if (HAS_ROT) D = {P.Dx[p], P.Dy[p], P.Dz[p]};
	tc_scale<HAS_ROT, LDS>(P, F, c, P.x[p], P.y[p], P.z[p], vx, vy, vz, D);
	P.vx[p] = vx; P.vy[p] = vy; P.vz[p] = vz;
	if (HAS_ROT) {
		P.Dx[p] = D.x; P.Dy[p] = D.y; P.Dz[p] = D.z;
	}
}

void launch_tc_apply(const TcParams& p, bool has_rot, uint32_t n_cap, hipStream_t s) {
	if (n_cap == 0 || p.nreg == 0) return;
	const dim3 grid((n_cap + TTPB - 1) / TTPB);
	const bool lds = p.total <= TC_APPLY_LDS_SLABS;
	if (has_rot) {
		if (lds) hipLaunchKernelGGL((k_tc_apply<true, true>), grid, dim3(TTPB), 0, s, p);
		else hipLaunchKernelGGL((k_tc_apply<true, false>), grid, dim3(TTPB), 0, s, p);
	} else {
		if (lds) hipLaunchKernelGGL((k_tc_apply<false, true>), grid, dim3(TTPB), 0, s, p);
		else hipLaunchKernelGGL((k_tc_apply<false, false>), grid, dim3(TTPB), 0, s, p);
	}
}

// The scaling of k_tc_apply on the values as they are read, then upd_preF (leap_pre of leapfrog_body.hpp: the arithmetic of
// k_kick_drift), the stores, the pair-stream record and the block maximum of the drift speed as k_kick_drift has them.  One
// workgroup per 256 molecules, as there: the displacement bound reads one maximum per workgroup of that size.
template <bool HAS_ROT, bool LDS>
__global__ void __launch_bounds__(TTPB) k_tc_kick_drift(IntegArgs a, TcParams P) {
	__shared__ double lfac[LDS ? TC_APPLY_LDS_SLABS : 1][2];
	tc_stage<LDS>(P, lfac);
	const TcFactors<LDS> F = {P.fac, lfac};
	const uint32_t p = blockIdx.x * TTPB + threadIdx.x;
	double v2 = 0.;
	if (p < a.cnt->n_real) {
		const int c = HAS_ROT ? a.mol.cid[p] : (a.ct->ncomp > 1 ? a.mol.cid[p] : 0);
		LeapState s;
		s.x = a.mol.x[p]; s.y = a.mol.y[p]; s.z = a.mol.z[p];
		s.vx = a.mol.vx[p]; s.vy = a.mol.vy[p]; s.vz = a.mol.vz[p];
		const V3 Fo = {a.frc.Fx[p], a.frc.Fy[p], a.frc.Fz[p]};
		V3 M = {0., 0., 0.}, invI = {0., 0., 0.};
		s.D = {0., 0., 0.};
		if (HAS_ROT) {
			s.q[0] = a.mol.q0[p]; s.q[1] = a.mol.q1[p]; s.q[2] = a.mol.q2[p]; s.q[3] = a.mol.q3[p];
			s.D = {a.mol.Dx[p], a.mol.Dy[p], a.mol.Dz[p]};
			M = {a.frc.Mx[p], a.frc.My[p], a.frc.Mz[p]};
			invI = {a.ct->invI[c][0], a.ct->invI[c][1], a.ct->invI[c][2]};
		}
		tc_scale<HAS_ROT, LDS>(P, F, c, s.x, s.y, s.z, s.vx, s.vy, s.vz, s.D);
		v2 = leap_pre<HAS_ROT>(a.dt, a.ct->mass[c], invI, Fo, M, s);
		a.mol.vx[p] = s.vx; a.mol.vy[p] = s.vy; a.mol.vz[p] = s.vz;
		a.mol.x[p] = s.x; a.mol.y[p] = s.y; a.mol.z[p] = s.z;
		if (HAS_ROT) {
			a.mol.q0[p] = s.q[0]; a.mol.q1[p] = s.q[1]; a.mol.q2[p] = s.q[2]; a.mol.q3[p] = s.q[3];
			a.mol.Dx[p] = s.D.x; a.mol.Dy[p] = s.D.y; a.mol.Dz[p] = s.D.z;
			if (a.pk) msl_write_record(a.pk, p, s.x, s.y, s.z, s.q[0], s.q[1], s.q[2], s.q[3], true, a.pk_ncomp > 1 ? c : 0);
		}
	}
	if (a.vmax_part) {  // (uniform) list mode: block maximum of |v_drift|^2 -> vmax_part[block]
		__shared__ double red[TTPB / 64];
		v2 = wave_fold_max(v2);
		if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v2;
		__syncthreads();
		if (threadIdx.x == 0) {
			double m = 0.;
			for (int i = 0; i < TTPB / 64; ++i) m = fmax(m, red[i]);
			a.vmax_part[blockIdx.x] = m;
		}
	}
}

void launch_tc_kick_drift(const IntegArgs& a, const TcParams& p, hipStream_t s) {
	if (a.n_cap == 0) return;
	const dim3 grid((a.n_cap + TTPB - 1) / TTPB);
	const bool lds = p.total <= TC_APPLY_LDS_SLABS;
	if (a.has_rot) {
		if (lds) hipLaunchKernelGGL((k_tc_kick_drift<true, true>), grid, dim3(TTPB), 0, s, a, p);
		else hipLaunchKernelGGL((k_tc_kick_drift<true, false>), grid, dim3(TTPB), 0, s, a, p);
	} else {
		if (lds) hipLaunchKernelGGL((k_tc_kick_drift<false, true>), grid, dim3(TTPB), 0, s, a, p);
		else hipLaunchKernelGGL((k_tc_kick_drift<false, false>), grid, dim3(TTPB), 0, s, a, p);
	}
}

}  // namespace ls1
