// molpair_energy.hpp — the energy half of the molecule-pair routine: what ParticlePairs2PotForceAdapter::processPair returns for a
// FLUIDPOT pair (particleContainer/adapter/ParticlePairs2PotForceAdapter.h:170-176), FluidPot
// (molecules/potforce.h:506-650) — Upot6LJ, UpotXpoles and MyRF of one molecule pair, no force, no torque, no
// virial.
//
// The same site loops, parameter products, shift6 and reaction-field term as mol_pair (molpair.hpp), every energy from the
// energy-only bodies of pairphys.hpp: the sum over the partners of a molecule equals what that molecule contributes to the U_pot
// the force kernels report.  Written out instead of calling mol_pair: the force and torque accumulators of the force form are
// what limits its occupancy, and nothing guarantees that a compiler removes them.
#pragma once
#include "molpair.hpp"

namespace ls1 {

struct PairU {
	double u6, uX, rf;  // 6 * U_LJ (shift included), multipole energy, reaction-field energy
};

// i: the test molecule, j: its partner; calcLJ: the centre distance is inside the LJ cutoff (as in mol_pair).
// CT, LJ_ONLY, ROT: as in mol_pair.
template <class CT = CompTable, bool LJ_ONLY = false, class ROT = Rot>
LS1_HD PairU mol_pair_energy(const CT& ct, int ci, V3 ri, const ROT& Ri, int cj, V3 rj, const ROT& Rj, bool calcLJ) {
	static_assert(LJ_ONLY || sizeof(ROT) == sizeof(Rot), "the axis form serves LJ-only component sets");
	double u6 = 0., uX = 0., rf = 0.;
	const int nlji = ct.nlj[ci], nljj = ct.nlj[cj];
	const int nci = LJ_ONLY ? 0 : ct.nc[ci], ncj = LJ_ONLY ? 0 : ct.nc[cj];
	const int ndi = LJ_ONLY ? 0 : ct.nd[ci], ndj = LJ_ONLY ? 0 : ct.nd[cj];
	const int nqi = LJ_ONLY ? 0 : ct.nq[ci], nqj = LJ_ONLY ? 0 : ct.nq[cj];
	if (calcLJ) {
		for (int si = 0; si < nlji; ++si) {
			const int gi = ct.olj[ci] + si;
			const V3 pi = ri + rotate(Ri, ld3(ct.ljpos, gi));
			for (int sj = 0; sj < nljj; ++sj) {
				const int gj = ct.olj[cj] + sj;
				const V3 dr = pi - (rj + rotate(Rj, ld3(ct.ljpos, gj)));
				const int k = gi * ct.ncenters + gj;
				u6 += lj_u6(dot(dr, dr), ct.eps24[k], ct.sig2[k]) + ct.shift6[k];
			}
		}
	}
	for (int si = 0; si < nci; ++si) {
		const int gi = ct.oc[ci] + si;
		const V3 pi = ri + rotate(Ri, ld3(ct.chpos, gi));
		const double qi = ct.chq[gi];
		for (int sj = 0; sj < ncj; ++sj) {  // charge-charge, potforce.h:556-565
			const int gj = ct.oc[cj] + sj;
			const V3 dr = pi - (rj + rotate(Rj, ld3(ct.chpos, gj)));
			uX += charge_charge_u(dot(dr, dr), qi * ct.chq[gj]);
		}
		for (int sj = 0; sj < nqj; ++sj) {  // charge-quadrupole
			const int gj = ct.oq[cj] + sj;
			const V3 dr = pi - (rj + rotate(Rj, ld3(ct.qppos, gj)));
			uX += charge_quadrupole_u(dr, dot(dr, dr), rotate(Rj, ld3(ct.qpe, gj)), 0.5 * qi * ct.qpQ[gj]);
		}
		for (int sj = 0; sj < ndj; ++sj) {  // charge-dipole
			const int gj = ct.od[cj] + sj;
			const V3 dr = pi - (rj + rotate(Rj, ld3(ct.dppos, gj)));
			uX += charge_dipole_u(dr, dot(dr, dr), rotate(Rj, ld3(ct.dpe, gj)), -qi * ct.dpmy[gj]);
		}
	}
	for (int si = 0; si < nqi; ++si) {
		const int gi = ct.oq[ci] + si;
		const V3 pi = ri + rotate(Ri, ld3(ct.qppos, gi));
		const V3 ei = rotate(Ri, ld3(ct.qpe, gi));
		const double Qi = ct.qpQ[gi];
		for (int sj = 0; sj < ncj; ++sj) {  // quadrupole-charge (roles swapped)
			const int gj = ct.oc[cj] + sj;
			const V3 dr = (rj + rotate(Rj, ld3(ct.chpos, gj))) - pi;
			uX += charge_quadrupole_u(dr, dot(dr, dr), ei, 0.5 * ct.chq[gj] * Qi);
		}
		for (int sj = 0; sj < nqj; ++sj) {  // quadrupole-quadrupole
			const int gj = ct.oq[cj] + sj;
			const V3 dr = pi - (rj + rotate(Rj, ld3(ct.qppos, gj)));
			uX += quadrupole_quadrupole_u(dr, dot(dr, dr), ei, rotate(Rj, ld3(ct.qpe, gj)), .75 * Qi * ct.qpQ[gj]);
		}
		for (int sj = 0; sj < ndj; ++sj) {  // quadrupole-dipole (roles swapped)
			const int gj = ct.od[cj] + sj;
			const V3 dr = (rj + rotate(Rj, ld3(ct.dppos, gj))) - pi;
			uX += dipole_quadrupole_u(dr, dot(dr, dr), rotate(Rj, ld3(ct.dpe, gj)), ei, 1.5 * Qi * ct.dpmy[gj]);
		}
	}
	for (int si = 0; si < ndi; ++si) {
		const int gi = ct.od[ci] + si;
		const V3 pi = ri + rotate(Ri, ld3(ct.dppos, gi));
		const V3 ei = rotate(Ri, ld3(ct.dpe, gi));
		const double myi = ct.dpmy[gi];
		for (int sj = 0; sj < ncj; ++sj) {  // dipole-charge (roles swapped)
			const int gj = ct.oc[cj] + sj;
			const V3 dr = (rj + rotate(Rj, ld3(ct.chpos, gj))) - pi;
			uX += charge_dipole_u(dr, dot(dr, dr), ei, -ct.chq[gj] * myi);
		}
		for (int sj = 0; sj < nqj; ++sj) {  // dipole-quadrupole
			const int gj = ct.oq[cj] + sj;
			const V3 dr = pi - (rj + rotate(Rj, ld3(ct.qppos, gj)));
			uX += dipole_quadrupole_u(dr, dot(dr, dr), ei, rotate(Rj, ld3(ct.qpe, gj)), 1.5 * myi * ct.qpQ[gj]);
		}
		for (int sj = 0; sj < ndj; ++sj) {  // dipole-dipole with the reaction field, potforce.h:36-80
			const int gj = ct.od[cj] + sj;
			const V3 dr = pi - (rj + rotate(Rj, ld3(ct.dppos, gj)));
			const double my2 = myi * ct.dpmy[gj];
			double rfp;
			uX += dipole_dipole_u(dr, dot(dr, dr), ei, rotate(Rj, ld3(ct.dpe, gj)), my2, my2 * ct.epsRFInvrc3, rfp);
			rf += rfp;
		}
	}
	return {u6, uX, rf};
}

}  // namespace ls1
