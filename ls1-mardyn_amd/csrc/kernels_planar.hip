// kernels_planar.hip — the planar long-range correction of vapour-liquid interfaces on the device: Planar::calculateLongRange with
// centerCenter / centerSite / siteSite / dipoleDipole (longRange/Planar.cpp:220-476, 479-1078), _smooth = false, restated as
//
//   k_planar_density  one pass over the OWNED molecules: u64 counts per (row, slab); rho = count slabs / V is formed when the tables
//                     are built.  Molecules are cell-sorted, so a workgroup's chunk spans a narrow y range: the histogram is kept
//                     in LDS (u32) when rows x slabs fits and only the touched slab range is flushed; else global atomics.
//   k_planar_kernels  the reference's slab-pair loops touch a pair of slabs only through its distance d (in slabs, 1 .. slabs -
//                     slabs / 2) and the branch d > cutoff_slabs: per ORDERED row pair the four kernels K_u, K_f, K_vN, K_vT(d);
//                     entry d = 0 is the pair's self term.
//   k_planar_tables   the O(rows^2 slabs^2) slab sum as a GATHER: a workgroup owns (output row, tile of 256 output slabs), a lane one
//                     output slab with four register accumulators; partner rows in ascending order, partner slabs in ascending
//                     order, no atomics: bit-reproducible.  rho of the partner row is staged in LDS in chunks of PL_CHUNK slabs (one
//                     broadcast read per trip), the two K blocks of the row pair (i-role and j-role) in LDS when they fit (stride-1
//                     reads), else they are read from global memory (neighbouring lanes read neighbouring d).
//   k_planar_apply    every step, one pass over the owned molecules: F_y, the torque d x f (lab frame, as the force kernels leave
//                     M), Vi, and {Upot_c, Virial_c} through per-workgroup partials folded by one workgroup in a fixed order.
#include <algorithm>

#include "common.hpp"

namespace ls1 {

constexpr int PLT = 256;               // threads per workgroup of every kernel here
constexpr uint32_t PL_PER_WG = 2048;   // molecules per workgroup of the density and the apply pass
constexpr uint32_t PL_LDS_BINS = 8192; // density: u32 histogram words in LDS (32 KB)
constexpr int PL_CHUNK = 512;          // tables: partner slabs staged per trip
constexpr int PL_K_LDS = 4096;         // tables: doubles of the two K blocks (2 x 4 x (nd + 1)) kept in LDS (32 KB)
constexpr uint32_t PL_TAB_LDS = 6144;  // apply: doubles of the four tables kept in LDS (48 KB)
uint32_t planar_apply_blocks(uint32_t n_cap) { return (n_cap + PL_PER_WG - 1) / PL_PER_WG; }

// (pl_wrap, the y wrap of every pass here: common.hpp — the wall pass shares it)
// slab of an LJ site (Planar.cpp:285-291): C truncation, one-slab wrap; clamped so that no index leaves the row
__device__ __forceinline__ int pl_site_slab(const PlanarParams& P, double y) {
	int loc = (int)(y * P.delta_inv);
	if (loc < 0) loc += P.slabs;
	else if (loc > P.slabs - 1) loc -= P.slabs;
	return min(max(loc, 0), P.slabs - 1);
}
// slab of a dipolar molecule's centre (:300); DEVIATION: a product that rounds to `slabs` at the upper face is clamped
__device__ __forceinline__ int pl_centre_slab(const PlanarParams& P, double y) { return min(max((int)(y * P.delta_inv), 0), P.slabs - 1); }

template <bool HAS_ROT>
__device__ __forceinline__ Rot pl_rot(const PlanarParams& P, uint32_t p) {
	if (!HAS_ROT) return rot_of(1., 0., 0., 0.);
	const double w = P.q0[p], x = P.q1[p], y = P.q2[p], z = P.q3[p];
	const double inv = 1. / sqrt(w * w + x * x + y * y + z * z);  // (normalised before rotating, as the force kernels do)
	return rot_of(w * inv, x * inv, y * inv, z * inv);
}

__global__ void __launch_bounds__(PLT) k_planar_clear(PlanarParams P) {
	const uint32_t w = blockIdx.x * PLT + threadIdx.x;
	if (w < (uint32_t)P.nrows * (uint32_t)P.slabs) P.counts[w] = 0ull;
}

template <bool HAS_ROT, bool LDS>
__global__ void __launch_bounds__(PLT) k_planar_density(PlanarParams P) {
	__shared__ uint32_t hist[LDS ? PL_LDS_BINS : 1];
	__shared__ int range[2];
	const uint32_t bins = (uint32_t)P.nrows * (uint32_t)P.slabs;
	if (LDS) {
		for (uint32_t w = threadIdx.x; w < bins; w += PLT) hist[w] = 0u;
		if (threadIdx.x == 0) {
			range[0] = P.slabs;
			range[1] = -1;
		}
		__syncthreads();
	}
	const uint32_t n = P.cnt->n_real;
	const uint32_t p0 = blockIdx.x * PL_PER_WG, p1 = min(p0 + PL_PER_WG, n);
	int lo = P.slabs, hi = -1;
	for (uint32_t p = p0 + threadIdx.x; p < p1; p += PLT) {
		const int c = P.ncomp > 1 ? P.cid[p] : 0;
		const double yc = pl_wrap(P.y[p], P.len_y);
		const int nlj = P.ct->nlj[c];
		if (nlj > 0) {
			const Rot R = pl_rot<HAS_ROT>(P, p);
			for (int s = 0; s < nlj; ++s) {
				const V3 d = rotate(R, ld3(P.ct->ljpos, P.ct->olj[c] + s));
				const int loc = pl_site_slab(P, yc + d.y);
				const uint32_t w = (uint32_t)(P.ljrow[c] + s) * (uint32_t)P.slabs + (uint32_t)loc;
				if (LDS) {
					atomicAdd(&hist[w], 1u);
					lo = min(lo, loc);
					hi = max(hi, loc);
				} else {
					atomicAdd(&P.counts[w], 1ull);
				}
			}
		}
		if (P.drow[c] >= 0) {
			const int loc = pl_centre_slab(P, yc);
			const uint32_t w = (uint32_t)(P.nlj + P.drow[c]) * (uint32_t)P.slabs + (uint32_t)loc;
			if (LDS) {
				atomicAdd(&hist[w], 1u);
				lo = min(lo, loc);
				hi = max(hi, loc);
			} else {
				atomicAdd(&P.counts[w], 1ull);
			}
		}
	}
	if (LDS) {
		if (hi >= 0) {
			atomicMin(&range[0], lo);
			atomicMax(&range[1], hi);
		}
		__syncthreads();
		const int r0 = range[0], width = range[1] - r0 + 1;  // touched slabs of every row (<= 0: nothing)
		if (width <= 0) return;
		for (uint32_t i = threadIdx.x; i < (uint32_t)P.nrows * (uint32_t)width; i += PLT) {
			const uint32_t row = i / (uint32_t)width, w = row * (uint32_t)P.slabs + (uint32_t)r0 + i % (uint32_t)width;
			const uint32_t v = hist[w];
			if (v) atomicAdd(&P.counts[w], (unsigned long long)v);
		}
	}
}

// K(d) of one ordered pair, d = 0 .. nd: what slab i receives per unit rho of slab j at distance d — u_i += rho_j K_u, vN_i += rho_j K_vN,
// vT_i += rho_j K_vT, f_i -= rho_j K_f in the DIRECT loops (+ in the periodic loop; slab j receives rho_i times the same with the
// force sign turned).  Entry d = 0 holds the pair's SELF term (K_u, K_vT per unit rho; :495-497, :621-622, :808-809): for centerSite
// and siteSite it is the inside-the-cutoff branch at r = 0.  pi = 3.1416 is the reference's.
__global__ void __launch_bounds__(PLT) k_planar_kernels(PlanarParams P, int npairs) {
	const int d = (int)(blockIdx.x * PLT + threadIdx.x), pair = (int)blockIdx.y;
	if (d > P.nd || pair >= npairs) return;
	const PlanarPair pp = P.pairs[pair];
	const double PI = 3.1416, delta = P.delta, cutoff = P.cutoff, sig = pp.sig, eps = pp.eps;
	const bool far = (double)d > P.cutoff_slabs;
	double Ku, Kf, KvN, KvT;
	if (pp.kind == PL_CC) {  // :479-523
		const double rc = sig / cutoff, rc2 = rc * rc, rc6 = rc2 * rc2 * rc2, rc12 = rc6 * rc6;
		const double termU = 4 * PI * delta * eps * sig * sig, termF = 8 * PI * delta * eps * sig, termVN = termU,
					 termVT = 2 * PI * delta * eps * sig * sig;
		const double r = sig / (d * delta);
		double r2, r6, r12;
		if (d == 0) {  // (r is infinite: the self term has its own expressions)
			r2 = rc2;
			r6 = rc6;
			r12 = rc12;
			KvT = termVT * (6 * rc12 * 0.2 - 3 * rc6 * 0.5) * (1.0 / rc2);
		} else if (far) {
			r2 = r * r;
			r6 = r2 * r2 * r2;
			r12 = r6 * r6;
			KvT = termVT * (r12 * 0.2 - r6 * 0.5) / r2;
		} else {
			r2 = rc2;
			r6 = rc6;
			r12 = rc12;
			KvT = termVT * (r12 * 0.2 * (6 / r2 - 5 / (r * r)) - r6 * 0.5 * (3 / r2 - 2 / (r * r)));
		}
		Ku = termU * (r12 * 0.2 - r6 * 0.5) / r2;
		KvN = d ? termVN * (r12 - r6) / (r * r) : 0.;
		Kf = d ? termF * (r12 - r6) / r : 0.;
		if (d == 0) Ku = termU * (rc12 * 0.2 - rc6 * 0.5) * (1.0 / rc2);
	} else if (pp.kind == PL_CS) {  // :590-663
		const double sig2 = sig * sig, sig3 = sig2 * sig, t = pp.t1 + pp.t2;
		const double r = d * delta, r2 = r * r, x = far ? r : cutoff;
		const double a = sig / (x + t), a3 = a * a * a, a4 = a3 * a, a9 = a3 * a3 * a3, a10 = a9 * a;
		const double b = sig / (x - t), b3 = b * b * b, b4 = b3 * b, b9 = b3 * b3 * b3, b10 = b9 * b;
		const double termU = -2 * PI * eps * delta * sig3 / (3 * t) * ((a9 - b9) / 15 - (a3 - b3) / 2);
		const double termF = -2 * PI * eps * delta * sig2 / (t * x) * ((a10 - b10) / 5 - (a4 - b4) / 2);
		Ku = termU;
		Kf = termF * r;
		KvN = termF / 2 * r2;
		if (far) {
			KvT = termU / 2;
		} else {
			const double vtrc1 = -PI * eps * delta * sig2 / (2 * t * x) * ((a10 - b10) / 5 - (a4 - b4) / 2);
			KvT = vtrc1 * (x * x - r2) + termU / 2;
		}
	} else if (pp.kind == PL_SS) {  // :763-860
		const double sig2 = sig * sig, sig3 = sig2 * sig, sig4 = sig2 * sig2, t1 = pp.t1, t2 = pp.t2, tP = t1 + t2, tM = t1 - t2;
		const double r = d * delta, r2 = r * r, x = far ? r : cutoff;
		const double a = sig / (x + tP), a2 = a * a, a3 = a2 * a, a8 = a2 * a3 * a3, a9 = a8 * a;
		const double b = sig / (x + tM), b2 = b * b, b3 = b2 * b, b8 = b2 * b3 * b3, b9 = b8 * b;
		const double e = sig / (x - tP), e2 = e * e, e3 = e2 * e, e8 = e2 * e3 * e3, e9 = e8 * e;
		const double g = sig / (x - tM), g2 = g * g, g3 = g2 * g, g8 = g2 * g3 * g3, g9 = g8 * g;
		const double termU = PI * eps * delta * sig4 / (12 * t1 * t2) * ((a8 - b8 - g8 + e8) / 30 - (a2 - b2 - g2 + e2));
		const double termF = PI * eps * delta * sig3 / (3 * t1 * t2 * x) * ((a9 - b9 - g9 + e9) / 15 - (a3 - b3 - g3 + e3) / 2);
		Ku = termU;
		Kf = termF * r;
		KvN = termF / 2 * r2;
		if (far) {
			KvT = termU / 2;
		} else {
			const double vtrc1 = PI * eps * delta * sig3 / (4 * t1 * t2 * x) * ((a9 - b9 - g9 + e9) / 45 - (a3 - b3 - g3 + e3) / 6);
			KvT = vtrc1 * (x * x - r2) + termU / 2;
		}
	} else {  // dipoleDipole, :980-1017; pp.sig = muSquare[ci] muSquare[cj] / (3 T)
		const double termU = PI / 4 * sig * delta, termF = PI * sig * delta, termVN = PI / 2 * sig * delta, termVT = termU;
		const double r = d * delta, x = far ? r : cutoff, x2 = x * x, x4 = x2 * x2, x6 = x4 * x2;
		Kf = -(termF / x6 * r);
		Ku = d ? -(termU / x4) : 0.;  // (no self term, :989-993)
		KvN = -(termVN / x6 * r * r);
		KvT = d ? -(termVT / x6 * (1.5 * x2 - r * r)) : 0.;
	}
	const int ks = P.nd + 1;
	double* const K = P.K + (size_t)pair * 4 * ks + d;
	K[0] = Ku;
	K[ks] = Kf;
	K[2 * ks] = KvN;
	K[3 * ks] = KvT;
}

// One launch per block of rows: LJ rows (row0 = 0, n = nlj, pair0 = 0) or dipole rows (row0 = nlj, n = ndip, pair0 = nlj^2).
// grid (tiles of PLT output slabs, n rows).
template <bool K_LDS>
__global__ void __launch_bounds__(PLT) k_planar_tables(PlanarParams P, int row0, int n, int pair0) {
	__shared__ double rho[PL_CHUNK];
	__shared__ double Ks[K_LDS ? PL_K_LDS : 1];
	const int A = (int)blockIdx.y, slabs = P.slabs, half = P.half, ks = P.nd + 1;
	const int k = (int)(blockIdx.x * PLT + threadIdx.x);
	const bool live = k < slabs;
	const size_t rs = (size_t)P.nrows * slabs;
	double u = 0., f = 0., vN = 0., vT = 0.;
	// self terms, entry d = 0 of the pair's K: centerCenter adds rho of its OWN row — in the right half to row self_row (:556-560;
	// outside the tables: dropped, the reference writes outside its arrays there) —, centerSite and siteSite rho of the partner row
	// at the same slab (:618-622, :805-809)
	if (live && pair0 == 0 && P.nlj > 0) {
		for (int pq = 0; pq < n * n; ++pq) {
			const PlanarPair pp = P.pairs[pq];
			const int Pi = pq / n, Q = pq % n, cc = pp.kind == PL_CC;
			const int dest = cc ? (k < half ? Pi : pp.self_row) : Pi, src = cc ? Pi : Q;
			if (dest != A) continue;
			const double* const K0 = P.K + (size_t)pq * 4 * ks;
			const double r = (double)P.counts[(size_t)src * slabs + k] * P.rho_unit;
			vT += K0[3 * ks] * r;
			u += K0[0] * r;
		}
	}
	for (int B = 0; B < n; ++B) {
		// K of the ordered pair (A, B): what A's slab receives as loop-i slab; of (B, A): what it receives as loop-j slab
		const double* const Ki = P.K + (size_t)(pair0 + A * n + B) * 4 * ks;
		const double* const Kj = P.K + (size_t)(pair0 + B * n + A) * 4 * ks;
		if (K_LDS) {
			__syncthreads();  // (the previous pair's blocks are no longer read)
			for (int w = threadIdx.x; w < 4 * ks; w += PLT) {
				Ks[w] = Ki[w];
				Ks[4 * ks + w] = Kj[w];
			}
		}
		const unsigned long long* const cB = P.counts + (size_t)(row0 + B) * slabs;
		for (int m0 = 0; m0 < slabs; m0 += PL_CHUNK) {
			const int mc = min(PL_CHUNK, slabs - m0);
			__syncthreads();
			for (int w = threadIdx.x; w < mc; w += PLT) rho[w] = (double)cB[m0 + w] * P.rho_unit;
			__syncthreads();
			if (!live) continue;
			for (int mm = 0; mm < mc; ++mm) {
				const int m = m0 + mm;
				if (m == k) continue;
				const bool is_i = k < m;  // this lane's slab is the pair's smaller index: loop-i role
				const int i = is_i ? k : m, j = is_i ? m : k;
				const bool direct = i >= half || j < i + half;
				const int d = direct ? j - i : slabs - j + i;
				const double r = rho[mm];
				const double* const Kp = K_LDS ? Ks + (is_i ? 0 : 4 * ks) + d : (is_i ? Ki : Kj) + d;
				u += r * Kp[0];
				const double rf = r * Kp[ks];
				f += (is_i == direct) ? -rf : rf;  // direct: f_i -= , f_j += ; periodic: the other way round
				vN += r * Kp[2 * ks];
				vT += r * Kp[3 * ks];
			}
		}
	}
	if (live) {
		const size_t o = (size_t)(row0 + A) * slabs + k;
		P.tab[o] = u;
		P.tab[rs + o] = f;
		P.tab[2 * rs + o] = vN;
		P.tab[3 * rs + o] = vT;
	}
}

template <bool HAS_ROT, bool LDS>
__global__ void __launch_bounds__(PLT) k_planar_apply(PlanarParams P) {
	__shared__ double tabs[LDS ? PL_TAB_LDS : 1];
	__shared__ double red[2][PLT / 64];
	const uint32_t rs = (uint32_t)P.nrows * (uint32_t)P.slabs;
	if (LDS) {
		for (uint32_t w = threadIdx.x; w < 4 * rs; w += PLT) tabs[w] = P.tab[w];
		__syncthreads();
	}
	const double* const tab = LDS ? tabs : P.tab;
	const uint32_t n = P.cnt->n_real;
	const uint32_t p0 = blockIdx.x * PL_PER_WG, p1 = min(p0 + PL_PER_WG, n);
	double up = 0., vir = 0.;
	for (uint32_t p = p0 + threadIdx.x; p < p1; p += PLT) {
		const int c = P.ncomp > 1 ? P.cid[p] : 0;
		const double yc = pl_wrap(P.y[p], P.len_y);
		const bool inside = yc >= P.region[0] && yc <= P.region[1];  // (:437) the force acts inside the region only
		double fy = 0., mx = 0., mz = 0., vt = 0., vn = 0.;
		const int nlj = P.ct->nlj[c];
		if (nlj > 0) {
			const Rot R = pl_rot<HAS_ROT>(P, p);
			for (int s = 0; s < nlj; ++s) {
				const V3 d = rotate(R, ld3(P.ct->ljpos, P.ct->olj[c] + s));
				const uint32_t o = (uint32_t)(P.ljrow[c] + s) * (uint32_t)P.slabs + (uint32_t)pl_site_slab(P, yc + d.y);
				const double f = tab[rs + o], tn = tab[2 * rs + o], tt = tab[3 * rs + o];
				up += tab[o];
				vir += 2 * tt + tn;
				vt += tt;
				vn += tn;
				if (inside) {
					fy += f;
					mx += -d.z * f;  // d x (0, f, 0)
					mz += d.x * f;
				}
			}
		}
		if (P.drow[c] >= 0) {  // (:443-457) on the centre of mass: no torque
			const uint32_t o = (uint32_t)(P.nlj + P.drow[c]) * (uint32_t)P.slabs + (uint32_t)pl_centre_slab(P, yc);
			const double tn = tab[2 * rs + o], tt = tab[3 * rs + o];
			up += tab[o];
			vir += 2 * tt + tn;
			vt += tt;
			vn += tn;
			if (inside) fy += tab[rs + o];
		}
		P.Fy[p] += fy;
		if (HAS_ROT) {
			P.Mx[p] += mx;
			P.Mz[p] += mz;
		}
		if (P.with_vi) {
			P.Vix[p] += vt;
			P.Viy[p] += vn;
			P.Viz[p] += vt;
		}
	}
	up = wave_fold_sum(up);
	vir = wave_fold_sum(vir);
	if ((threadIdx.x & 63) == 0) {
		red[0][threadIdx.x >> 6] = up;
		red[1][threadIdx.x >> 6] = vir;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		double a = 0., b = 0.;
		for (int w = 0; w < PLT / 64; ++w) {
			a += red[0][w];
			b += red[1][w];
		}
		P.partials[2 * blockIdx.x] = a;
		P.partials[2 * blockIdx.x + 1] = b;
	}
}

// {Upot_c, Virial_c}: the workgroups' partials folded by ONE workgroup, lane l taking partials l, l + 256, ... in ascending order
__global__ void __launch_bounds__(PLT) k_planar_reduce(PlanarParams P, uint32_t nb_cap) {
	__shared__ double red[2][PLT / 64];
	const uint32_t nb = min(nb_cap, (P.cnt->n_real + PL_PER_WG - 1) / PL_PER_WG);
	double a = 0., b = 0.;
	for (uint32_t i = threadIdx.x; i < nb; i += PLT) {
		a += P.partials[2 * i];
		b += P.partials[2 * i + 1];
	}
	a = wave_fold_sum(a);
	b = wave_fold_sum(b);
	if ((threadIdx.x & 63) == 0) {
		red[0][threadIdx.x >> 6] = a;
		red[1][threadIdx.x >> 6] = b;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		a = b = 0.;
		for (int w = 0; w < PLT / 64; ++w) {
			a += red[0][w];
			b += red[1][w];
		}
		P.out2[0] = a;
		P.out2[1] = b;
		if (P.log2) {
			P.log2[0] = a;
			P.log2[1] = b;
		}
	}
}

void launch_planar_clear(const PlanarParams& p, hipStream_t s) {
	const uint32_t bins = (uint32_t)p.nrows * (uint32_t)p.slabs;
	hipLaunchKernelGGL(k_planar_clear, dim3((bins + PLT - 1) / PLT), dim3(PLT), 0, s, p);
}

void launch_planar_density(const PlanarParams& p, bool has_rot, uint32_t n_cap, hipStream_t s) {
	if (n_cap == 0) return;
	const dim3 grid((n_cap + PL_PER_WG - 1) / PL_PER_WG);
	const bool lds = (size_t)p.nrows * p.slabs <= PL_LDS_BINS;
	if (has_rot) {
		if (lds) hipLaunchKernelGGL((k_planar_density<true, true>), grid, dim3(PLT), 0, s, p);
		else hipLaunchKernelGGL((k_planar_density<true, false>), grid, dim3(PLT), 0, s, p);
	} else {
		if (lds) hipLaunchKernelGGL((k_planar_density<false, true>), grid, dim3(PLT), 0, s, p);
		else hipLaunchKernelGGL((k_planar_density<false, false>), grid, dim3(PLT), 0, s, p);
	}
}

void launch_planar_tables(const PlanarParams& p, hipStream_t s) {
	const int npairs = p.nlj * p.nlj + p.ndip * p.ndip;
	if (npairs == 0) return;
	hipLaunchKernelGGL(k_planar_kernels, dim3((p.nd + 1 + PLT - 1) / PLT, npairs), dim3(PLT), 0, s, p, npairs);
	const bool k_lds = 8 * (p.nd + 1) <= PL_K_LDS;
	const uint32_t tiles = (p.slabs + PLT - 1) / PLT;
	for (int blk = 0; blk < 2; ++blk) {
		const int row0 = blk ? p.nlj : 0, n = blk ? p.ndip : p.nlj, pair0 = blk ? p.nlj * p.nlj : 0;
		if (n == 0) continue;
		if (k_lds) hipLaunchKernelGGL((k_planar_tables<true>), dim3(tiles, n), dim3(PLT), 0, s, p, row0, n, pair0);
		else hipLaunchKernelGGL((k_planar_tables<false>), dim3(tiles, n), dim3(PLT), 0, s, p, row0, n, pair0);
	}
}

void launch_planar_apply(const PlanarParams& p, bool has_rot, uint32_t n_cap, hipStream_t s) {
	const uint32_t nb = planar_apply_blocks(n_cap);
	if (nb) {
		const bool lds = (size_t)4 * p.nrows * p.slabs <= PL_TAB_LDS;
		if (has_rot) {
			if (lds) hipLaunchKernelGGL((k_planar_apply<true, true>), dim3(nb), dim3(PLT), 0, s, p);
			else hipLaunchKernelGGL((k_planar_apply<true, false>), dim3(nb), dim3(PLT), 0, s, p);
		} else {
			if (lds) hipLaunchKernelGGL((k_planar_apply<false, true>), dim3(nb), dim3(PLT), 0, s, p);
			else hipLaunchKernelGGL((k_planar_apply<false, false>), dim3(nb), dim3(PLT), 0, s, p);
		}
	}
	hipLaunchKernelGGL(k_planar_reduce, dim3(1), dim3(PLT), 0, s, p, nb);
}

}  // namespace ls1
