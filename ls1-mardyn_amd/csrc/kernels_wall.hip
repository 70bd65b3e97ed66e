// kernels_wall.hip — the external fields that close a film, an adsorption or an evaporation set-up in y, on the device: the integrated
// Lennard-Jones wall of plugins/WallPotential.cpp (calcTSLJ_9_3 :193-258, calcTSLJ_10_4 :264-341) and the planes of plugins/Mirror.cpp
// (VelocityChange :421-477: MT_REFLECT, MT_FORCE_CONSTANT), restated as ONE pass over the owned molecules, a sibling of k_planar_apply:
//
//   k_wall_apply   a workgroup owns WL_PER_WG consecutive molecules.  Molecules are cell-sorted, so that chunk spans a narrow y range
//                  and most workgroups see no wall and no mirror at all.  The pass is therefore built around what it does NOT read:
//                    1. every lane loads the y of its WL_ITER molecules (8 B each; all loads in flight at once) and tests it against
//                       the conservative reach of the wall (site offsets of at most d_max included) and the mirror regions;
//                    2. a workgroup without any hit writes its zero partials and ends: no cid, no quaternion, no F, no v;
//                    3. the others stage the per-component wall constants in LDS (a lane per component) and walk their molecules
//                       again; a wave whose ballot of hits is empty in an iteration skips it without a load.  Lanes that hit load
//                       cid (and the quaternion unless the component is a single centred site), walk the LJ sites as
//                       k_planar_apply does, and read-modify-write Fy (Mx, Mz) only if a site really was inside ycut, vy only if
//                       a mirror flipped it: every other molecule keeps F, M and v bit for bit;
//                    4. per-component energies: per-lane register accumulators (MAXC = 8: the component cap of the library is the
//                       cap of this pass) -> wave_fold_sum -> per-workgroup partials.
//   k_wall_reduce  one workgroup folds the partials in ascending order (the scheme of k_planar_reduce): bit-reproducible energies.
//
// The wall energy is Sum over sites of (u - u_shift) per component; the reference keeps it in Domain::setLocalUpotCompSpecific only, it
// never enters U_pot or the virial — here it has an output of its own.  DEVIATION: the 10-4-3 energy and its shift use 2./5.; the
// reference's integer 2 / 5 is 0 (:184, :318).  No output of the reference shows that energy.
#include "common.hpp"

namespace ls1 {

constexpr int WLT = 256;              // threads per workgroup
constexpr int WL_ITER = 8;            // molecules per lane
constexpr uint32_t WL_PER_WG = WLT * WL_ITER;  // 2048, the chunk of the planar apply pass
uint32_t wall_apply_blocks(uint32_t n_cap) { return (n_cap + WL_PER_WG - 1) / WL_PER_WG; }

constexpr unsigned WL_HIT_WALL = 1u, WL_HIT_MIRROR = 2u;  // per molecule, two bits of the lane's hit word

// Mirror::VelocityChange's region (:429-443) through the half-open test of MoleculeInterface::inBox (r >= low and r < high) on the
// wrapped centre, which lies in [0, L): a right mirror o-| owns [coord, L), a left mirror |-o owns [0, coord)
__device__ __forceinline__ bool wl_in_mirror(const WallMirror& m, double y) { return m.dir ? y >= m.coord : y < m.coord; }

template <bool HAS_ROT>
__global__ void __launch_bounds__(WLT) k_wall_apply(WallParams P) {
	__shared__ WallComp comp[MAXC];
	__shared__ double red[MAXC][WLT / 64];
	const uint32_t n = P.cnt->n_real;
	const uint32_t p0 = blockIdx.x * WL_PER_WG + threadIdx.x;
	// 1. y only
	double yc[WL_ITER];
	unsigned hits = 0;
#pragma unroll
	for (int i = 0; i < WL_ITER; ++i) {
		const uint32_t p = p0 + i * WLT;
		yc[i] = 0.;
		if (p >= n) continue;
		const double y = pl_wrap(P.y[p], P.len_y);
		yc[i] = y;
		unsigned h = (P.potential != WL_OFF && y >= P.reach[0] && y <= P.reach[1]) ? WL_HIT_WALL : 0u;
#pragma unroll
		for (int m = 0; m < WL_MIRRORS; ++m)
			if (P.mir[m].type != WL_MT_OFF && wl_in_mirror(P.mir[m], y)) h |= WL_HIT_MIRROR;
		hits |= h << (2 * i);
	}
	// 2. nobody in reach of anything: zero partials, nothing else
	if (!__syncthreads_or((int)hits)) {
		if ((int)threadIdx.x < P.ncomp) P.partials[(size_t)blockIdx.x * MAXC + threadIdx.x] = 0.;
		return;
	}
	// 3. constants to LDS, then the molecules in reach
	if ((int)threadIdx.x < P.ncomp) comp[threadIdx.x] = P.comp[threadIdx.x];
	__syncthreads();
	double e[MAXC];
#pragma unroll
	for (int k = 0; k < MAXC; ++k) e[k] = 0.;
#pragma unroll
	for (int i = 0; i < WL_ITER; ++i) {
		const unsigned h = (hits >> (2 * i)) & 3u;
		if (__ballot(h != 0) == 0) continue;  // the whole wave is out of reach: no load
		if (h == 0) continue;
		const uint32_t p = p0 + i * WLT;
		const double y = yc[i];
		const int c = P.ncomp > 1 ? P.cid[p] : 0;
		double fy = 0., mx = 0., mz = 0., du = 0.;
		bool touched = false;
		if ((h & WL_HIT_WALL) && comp[c].consider) {
			const WallComp W = comp[c];
			const bool rot = HAS_ROT && !W.centre;
			const Rot R = rot ? rot_of_stored(P.q0[p], P.q1[p], P.q2[p], P.q3[p]) : rot_of(1., 0., 0., 0.);
			const int nlj = P.ct->nlj[c], o = P.ct->olj[c];
			for (int s = 0; s < nlj; ++s) {
				const V3 d = W.centre ? V3{0., 0., 0.} : rotate(R, ld3(P.ct->ljpos, o + s));
				const double ry = y + d.y;  // ljcenter_d_abs
				const double ryRel = (ry > P.yoff) ? (ry - (P.yoff + P.whalf)) : (ry - (P.yoff - P.whalf));  // :223, :295
				const double ya = fabs(ryRel);
				if (!(ya < P.ycut)) continue;
				double f, u;
				if (P.potential == WL_93) {  // :228-242
					const double y3 = ya * ya * ya, y9 = y3 * y3 * y3;
					f = W.pref * (W.b / 5.0 / y9 - W.a / 2.0 / y3) / ya;
					u = W.pref * (W.b / 45.0 / y9 - W.a / 6.0 / y3) - W.ushift;
				} else {  // :298-319
					const double y2 = ya * ya, y4 = y2 * y2, y5 = y4 * ya, y10 = y5 * y5, y11 = y10 * ya;
					const double bracket = ya + P.delta061, bracket3 = bracket * bracket * bracket;
					const double term1 = W.b / y10, term2 = W.a / y4, term3 = W.a / (P.delta3 * bracket3);
					u = W.pref * ((2. / 5.) * term1 - term2 - term3) - W.ushift;
					f = W.pref * (4 * (W.b / y11) - 4 * (W.a / y5) - term3 * 3 / bracket);
				}
				if (ryRel < 0) f = -f;
				fy += f;
				mx += -d.z * f;  // d x (0, f, 0), lab frame
				mz += d.x * f;
				du += u;
				touched = true;
			}
		}
		bool torque = touched && HAS_ROT && !comp[c].centre;
		if (h & WL_HIT_MIRROR) {
			bool loaded = false;
			double v0 = 0., v = 0.;
#pragma unroll
			for (int m = 0; m < WL_MIRRORS; ++m) {
				const WallMirror& M = P.mir[m];
				if (M.type == WL_MT_OFF || !wl_in_mirror(M, y) || (M.cid != 0 && c + 1 != M.cid)) continue;  // :457
				if (M.type == WL_MT_REFLECT) {  // :459-463
					if (!loaded) {
						v0 = v = P.vy[p];
						loaded = true;
					}
					if ((M.dir == 1 && v > 0.) || (M.dir == 0 && v < 0.)) v = -v;
				} else {  // MT_FORCE_CONSTANT, :464-473: on the centre of mass, no torque
					fy += M.k * (M.coord - y);
					touched = true;
				}
			}
			if (loaded && v != v0) P.vy[p] = v;
		}
		if (touched) P.Fy[p] += fy;
		if (torque) {
			P.Mx[p] += mx;
			P.Mz[p] += mz;
		}
#pragma unroll
		for (int k = 0; k < MAXC; ++k) e[k] += (c == k) ? du : 0.;
	}
	// 4. per-component energies of the workgroup
#pragma unroll
	for (int k = 0; k < MAXC; ++k) {
		if (k >= P.ncomp) break;
		const double w = wave_fold_sum(e[k]);
		if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = w;
	}
	__syncthreads();
	if ((int)threadIdx.x < P.ncomp) {
		double a = 0.;
		for (int w = 0; w < WLT / 64; ++w) a += red[threadIdx.x][w];
		P.partials[(size_t)blockIdx.x * MAXC + threadIdx.x] = a;
	}
}

// per-component energies: the workgroups' partials folded by ONE workgroup, lane l taking partials l, l + 256, ... in ascending order
__global__ void __launch_bounds__(WLT) k_wall_reduce(WallParams P, uint32_t nb_cap) {
	__shared__ double red[MAXC][WLT / 64];
	const uint32_t nb = min(nb_cap, (P.cnt->n_real + WL_PER_WG - 1) / WL_PER_WG);
	for (int k = 0; k < P.ncomp; ++k) {
		double a = 0.;
		for (uint32_t i = threadIdx.x; i < nb; i += WLT) a += P.partials[(size_t)i * MAXC + k];
		a = wave_fold_sum(a);
		if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = a;
	}
	__syncthreads();
	if (threadIdx.x < MAXC) {
		double a = 0.;
		if ((int)threadIdx.x < P.ncomp)
			for (int w = 0; w < WLT / 64; ++w) a += red[threadIdx.x][w];
		P.out[threadIdx.x] = a;
		if (P.log) P.log[threadIdx.x] = a;
	}
}

void launch_wall_apply(const WallParams& p, bool has_rot, uint32_t n_cap, hipStream_t s) {
	const uint32_t nb = wall_apply_blocks(n_cap);
	if (nb) {
		if (has_rot) hipLaunchKernelGGL((k_wall_apply<true>), dim3(nb), dim3(WLT), 0, s, p);
		else hipLaunchKernelGGL((k_wall_apply<false>), dim3(nb), dim3(WLT), 0, s, p);
	}
	hipLaunchKernelGGL(k_wall_reduce, dim3(1), dim3(WLT), 0, s, p, nb);
}

}  // namespace ls1
