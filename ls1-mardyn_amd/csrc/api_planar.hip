// api_planar.hip — the C ABI of libls1hip (include/ls1hip.h), part 6: the planar long-range correction of vapour-liquid interfaces
// (the reference's longRange/Planar.{h,cpp}), kernels in kernels_planar.hip.
#include "api_internal.hpp"

static void planar_free(ls1hip_ctx* c) {
	dfree(c->d_pl_counts);
	dfree(c->d_pl_pairs);
	dfree(c->d_pl_K);
	dfree(c->d_pl_tab);
	dfree(c->d_pl_partials);
	dfree(c->d_pl_out);
	dfree(c->d_pl_log);
	c->pl_partials_cap = 0;
	c->pl = PlanarParams{};
	c->pl_calls = 0;
	c->pl_tables_valid = false;
}

void planar_destroy(ls1hip_ctx* c) { planar_free(c); }

// Planar::init (Planar.cpp:40-157): rows, elongations, muSquare, slab geometry; the ordered pairs of calculateLongRange (:338-371)
extern "C" int ls1hip_planar_config(ls1hip_ctx* c, int slabs, int frequency, double region_left, double region_right, double temperature) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, slabs >= 0, "slabs must be >= 0 (0 switches the correction off), got %d", slabs);
	if (slabs == 0) {
		if (c->pl.slabs) {
			HIPCHK(c, hipSetDevice(c->device));
			HIPCHK(c, hipStreamSynchronize(c->stream));
		}
		planar_free(c);
		return LS1HIP_OK;
	}
	REQUIRE(c, c->have_comp && c->have_domain, "ls1hip_planar_config needs the components and the domain (ls1hip_set_components, ls1hip_set_domain)");
	REQUIRE(c, slabs >= 2, "at least 2 slabs, got %d", slabs);
	REQUIRE(c, frequency >= 1, "frequency must be >= 1, got %d", frequency);
	REQUIRE(c, region_left <= region_right, "region [%g, %g] is empty", region_left, region_right);
	const CompTable& ct = c->h_ct;
	PlanarParams P{};
	P.slabs = slabs;
	P.ncomp = ct.ncomp;
	bool gap = false;
	for (int k = 0; k < ct.ncomp; ++k) {
		P.ljrow[k] = P.nlj;
		P.nlj += ct.nlj[k];
		const bool dip = ct.nd[k] > 0 || ct.nc[k] != 0;
		// dipoleDipole reads muSquare[ci] by COMPONENT id from an array filled in order of the dipolar components (:126, :985): the two
		// agree only while no component without dipole / charge precedes one with; the reference reads outside its array otherwise
		REQUIRE(c, !(dip && gap), "component %d has dipoles / charges but an earlier component has none: not served (Planar::dipoleDipole)", k);
		if (!dip) gap = true;
		P.drow[k] = dip ? P.ndip++ : -1;
	}
	REQUIRE(c, P.ndip == 0 || temperature > 0., "dipolar components need the target temperature > 0, got %g", temperature);
	P.nrows = P.nlj + P.ndip;
	REQUIRE(c, P.nrows > 0, "no LJ site and no dipolar component");
	REQUIRE(c, (double)P.nrows * slabs * 4 < 2147483647., "tables of %d rows x %d slabs exceed the 32-bit index", P.nrows, slabs);
	P.half = slabs / 2;
	P.nd = slabs - P.half;
	P.len_y = c->global_len[1];
	P.cutoff = c->rc_lj;
	P.cutoff_slabs = P.cutoff * slabs / P.len_y;
	P.delta = P.len_y / slabs;
	P.delta_inv = 1.0 / P.delta;
	P.rho_unit = slabs / (P.len_y * c->global_len[0] * c->global_len[2]);
	P.region[0] = region_left;
	P.region[1] = region_right;
	// ordered pairs: LJ rows [nlj][nlj], then dipole rows [ndip][ndip]
	std::vector<PlanarPair> pairs((size_t)P.nlj * P.nlj + (size_t)P.ndip * P.ndip);
	std::vector<double> elong(P.nlj);
	std::vector<int> comp_of(P.nlj), site_of(P.nlj);
	for (int k = 0; k < ct.ncomp; ++k)
		for (int s = 0; s < ct.nlj[k]; ++s) {
			const double* d = ct.ljpos[ct.olj[k] + s];
			elong[P.ljrow[k] + s] = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
			comp_of[P.ljrow[k] + s] = k;
			site_of[P.ljrow[k] + s] = s;
		}
	for (int a = 0; a < P.nlj; ++a)
		for (int b = 0; b < P.nlj; ++b) {
			PlanarPair& pp = pairs[(size_t)a * P.nlj + b];
			const int ga = ct.olj[comp_of[a]] + site_of[a], gb = ct.olj[comp_of[b]] + site_of[b];
			pp.sig = sqrt(ct.sig2[ga * ct.ncenters + gb]);
			pp.eps = ct.eps24[ga * ct.ncenters + gb] / 24;
			pp.t1 = elong[a];
			pp.t2 = elong[b];
			pp.kind = (elong[a] == 0 && elong[b] == 0) ? PL_CC : (elong[a] == 0 || elong[b] == 0) ? PL_CS : PL_SS;
			// tau > r_c - delta makes sig / (r - tau) of centerSite / siteSite singular inside the tabulated range
			REQUIRE(c, pp.kind == PL_CC || pp.t1 + pp.t2 < P.cutoff, "site elongations %g + %g reach the cutoff %g", pp.t1, pp.t2, P.cutoff);
			const int sr = P.ljrow[comp_of[b]] + site_of[a];  // index_i_cj of centerCenter (:556)
			pp.self_row = sr < P.nlj ? sr : -1;
		}
	std::vector<double> mu2(P.ndip, 0.);
	for (int k = 0; k < ct.ncomp; ++k) {
		if (P.drow[k] < 0) continue;
		double cb[3] = {0, 0, 0};  // chargeBalance (:112-126)
		for (int s = 0; s < ct.nc[k]; ++s)
			for (int d = 0; d < 3; ++d) cb[d] += ct.chq[ct.oc[k] + s] * ct.chpos[ct.oc[k] + s][d];
		for (int s = 0; s < ct.nd[k]; ++s)
			for (int d = 0; d < 3; ++d) cb[d] += ct.dpmy[ct.od[k] + s] * ct.dpe[ct.od[k] + s][d];
		mu2[P.drow[k]] = cb[0] * cb[0] + cb[1] * cb[1] + cb[2] * cb[2];
	}
	for (int a = 0; a < P.ndip; ++a)
		for (int b = 0; b < P.ndip; ++b) {
			PlanarPair& pp = pairs[(size_t)P.nlj * P.nlj + (size_t)a * P.ndip + b];
			pp.kind = PL_DD;
			pp.self_row = -1;
			pp.sig = mu2[a] * mu2[b] / (3 * temperature);
			pp.eps = pp.t1 = pp.t2 = 0.;
		}
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	planar_free(c);
	const size_t rs = (size_t)P.nrows * slabs;
	int rc;
	if ((rc = dalloc(c, &c->d_pl_counts, rs)) || (rc = dalloc(c, &c->d_pl_pairs, pairs.size())) ||
		(rc = dalloc(c, &c->d_pl_K, pairs.size() * 4 * (P.nd + 1))) || (rc = dalloc(c, &c->d_pl_tab, 4 * rs)) || (rc = dalloc(c, &c->d_pl_out, 2)) ||
		(rc = dalloc(c, &c->d_pl_log, STEPLOG_ROWS * 2))) {
		planar_free(c);
		return rc;
	}
	HIPCHK(c, hipMemcpy(c->d_pl_pairs, pairs.data(), pairs.size() * sizeof(PlanarPair), hipMemcpyHostToDevice));
	HIPCHK(c, hipMemset(c->d_pl_counts, 0, rs * sizeof(unsigned long long)));
	HIPCHK(c, hipMemset(c->d_pl_tab, 0, 4 * rs * sizeof(double)));
	HIPCHK(c, hipMemset(c->d_pl_out, 0, 2 * sizeof(double)));
	c->pl = P;
	c->pl_frequency = frequency;
	return LS1HIP_OK;
}

// the kernel arguments of the current state; molecules: the pass reads the molecules (and the state must allow it)
static int planar_params(ls1hip_ctx* c, PlanarParams& P, bool molecules) {
	REQUIRE(c, c->pl.slabs > 0 && c->d_pl_counts, "the planar correction is not configured (ls1hip_planar_config)");
	P = c->pl;
	P.counts = c->d_pl_counts;
	P.pairs = c->d_pl_pairs;
	P.K = c->d_pl_K;
	P.tab = c->d_pl_tab;
	P.out2 = c->d_pl_out;
	P.ct = c->d_ct;
	P.cnt = c->d_cnt;
	if (!molecules) return LS1HIP_OK;
	REQUIRE(c, c->cap_real, "no molecules uploaded");
	REQUIRE(c, !c->fused_split && !c->inner_in_flight, "a split force pass is in flight");
	REQUIRE(c, !c->half_advanced && c->pos_x != c->frc.Fx,
			"the state was advanced by a fused force + integration pass (the correction follows an unfused force pass)");
	REQUIRE(c, c->pl.ncomp == c->h_ct.ncomp, "the component set changed since ls1hip_planar_config");
	const MolSoA& m = c->mol[c->cur];
	const Pos3 r = cur_pos(c);
	P.x = r.x; P.y = r.y; P.z = r.z;
	P.q0 = m.q0; P.q1 = m.q1; P.q2 = m.q2; P.q3 = m.q3;
	P.cid = m.cid;
	P.Fy = c->frc.Fy; P.Mx = c->frc.Mx; P.Mz = c->frc.Mz;
	P.Vix = c->frc.Vix; P.Viy = c->frc.Viy; P.Viz = c->frc.Viz;
	P.with_vi = c->opt_vi ? 1 : 0;
	return LS1HIP_OK;
}

static int planar_density_impl(ls1hip_ctx* c, bool clear) {
	PlanarParams P;
	int rc = planar_params(c, P, true);
	if (rc) return rc;
	TimedScope ts(c, c->t_pl_density);
	if (clear) launch_planar_clear(P, c->stream);
	launch_planar_density(P, c->h_ct.has_rot != 0, (uint32_t)c->n_real, c->stream);
	HIPCHK(c, hipGetLastError());
	return LS1HIP_OK;
}

static int planar_tables_impl(ls1hip_ctx* c) {
	PlanarParams P;
	int rc = planar_params(c, P, false);
	if (rc) return rc;
	TimedScope ts(c, c->t_pl_tables);
	launch_planar_tables(P, c->stream);
	HIPCHK(c, hipGetLastError());
	c->pl_tables_valid = true;
	return LS1HIP_OK;
}

static int planar_apply_impl(ls1hip_ctx* c, double* log2) {
	PlanarParams P;
	int rc = planar_params(c, P, true);
	if (rc) return rc;
	REQUIRE(c, c->pl_tables_valid, "no tables yet (ls1hip_planar_tables)");
	REQUIRE(c, c->forces_valid, "the correction is added to valid forces (ls1hip_forces)");
	const uint32_t nb = planar_apply_blocks((uint32_t)c->n_real);
	if (nb > c->pl_partials_cap) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		dfree(c->d_pl_partials);
		if ((rc = dalloc(c, &c->d_pl_partials, (size_t)2 * nb))) return rc;
		c->pl_partials_cap = nb;
	}
	P.partials = c->d_pl_partials;
	P.log2 = log2;
	TimedScope ts(c, c->t_pl_apply);
	launch_planar_apply(P, c->h_ct.has_rot != 0, (uint32_t)c->n_real, c->stream);
	HIPCHK(c, hipGetLastError());
	return LS1HIP_OK;
}

static int planar_result(ls1hip_ctx* c, double* upot_corr, double* virial_corr) {
	if (!upot_corr && !virial_corr) return LS1HIP_OK;
	double h[2];
	HIPCHK(c, hipMemcpyAsync(h, c->d_pl_out, sizeof(h), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (upot_corr) *upot_corr = h[0];
	if (virial_corr) *virial_corr = h[1];
	return LS1HIP_OK;
}

int planar_impl(ls1hip_ctx* c, double* log2) {
	REQUIRE(c, c->pl.slabs > 0, "the planar correction is not configured (ls1hip_planar_config)");
	REQUIRE(c, c->forces_valid, "the correction is added to valid forces (ls1hip_forces)");
	int rc;
	if (c->pl_calls % (unsigned long)c->pl_frequency == 0) {  // simstep % frequency == 0 (:259)
		if ((rc = planar_density_impl(c, true)) || (rc = planar_tables_impl(c))) return rc;
	}
	if ((rc = planar_apply_impl(c, log2))) return rc;
	c->pl_calls++;
	return LS1HIP_OK;
}

extern "C" int ls1hip_long_range_planar(ls1hip_ctx* c, double* upot_corr, double* virial_corr) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, !c->has_remote, "ls1hip_long_range_planar is the single-rank form (multi-rank: planar_density / counts / tables / apply)");
	HIPCHK(c, hipSetDevice(c->device));
	int rc = planar_impl(c, nullptr);
	if (rc) return rc;
	return planar_result(c, upot_corr, virial_corr);
}

extern "C" int ls1hip_planar_density(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	return planar_density_impl(c, false);
}

extern "C" int ls1hip_planar_counts_read(ls1hip_ctx* c, size_t cap, uint64_t* counts) {
	if (!c || !counts) return LS1HIP_EINVAL;
	REQUIRE(c, c->pl.slabs > 0 && c->d_pl_counts, "the planar correction is not configured (ls1hip_planar_config)");
	const size_t rs = (size_t)c->pl.nrows * c->pl.slabs;
	REQUIRE(c, cap >= rs, "buffer too small: %zu < %zu counts", cap, rs);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(counts, c->d_pl_counts, rs * 8, hipMemcpyDeviceToHost));
	return LS1HIP_OK;
}

extern "C" int ls1hip_planar_counts_write(ls1hip_ctx* c, size_t n, const uint64_t* counts) {
	if (!c || !counts) return LS1HIP_EINVAL;
	REQUIRE(c, c->pl.slabs > 0 && c->d_pl_counts, "the planar correction is not configured (ls1hip_planar_config)");
	const size_t rs = (size_t)c->pl.nrows * c->pl.slabs;
	REQUIRE(c, n == rs, "%zu counts given, the layout has %zu", n, rs);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(c->d_pl_counts, counts, rs * 8, hipMemcpyHostToDevice));
	return LS1HIP_OK;
}

extern "C" int ls1hip_planar_tables(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	return planar_tables_impl(c);
}

extern "C" int ls1hip_planar_apply(ls1hip_ctx* c, double* upot_corr, double* virial_corr) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	int rc = planar_apply_impl(c, nullptr);
	if (rc) return rc;
	return planar_result(c, upot_corr, virial_corr);
}

extern "C" int ls1hip_planar_read(ls1hip_ctx* c, int layout[3], size_t cap, double* rho, double* u, double* vN, double* vT, double* f) {
	if (!c) return LS1HIP_EINVAL;
	if (layout) {
		layout[0] = c->pl.slabs;
		layout[1] = c->pl.nlj;
		layout[2] = c->pl.ndip;
	}
	if (!(rho || u || vN || vT || f)) return LS1HIP_OK;
	REQUIRE(c, c->pl.slabs > 0 && c->d_pl_counts, "the planar correction is not configured (ls1hip_planar_config)");
	const size_t rs = (size_t)c->pl.nrows * c->pl.slabs;
	REQUIRE(c, cap >= rs, "buffers too small: %zu < %zu entries", cap, rs);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (rho) {
		std::vector<unsigned long long> cnt(rs);
		HIPCHK(c, hipMemcpy(cnt.data(), c->d_pl_counts, rs * 8, hipMemcpyDeviceToHost));
		for (size_t i = 0; i < rs; ++i) rho[i] = (double)cnt[i] * c->pl.rho_unit;
	}
	double* const dst[4] = {u, f, vN, vT};  // device order of PlanarParams::tab
	for (int k = 0; k < 4; ++k)
		if (dst[k]) HIPCHK(c, hipMemcpy(dst[k], c->d_pl_tab + k * rs, rs * 8, hipMemcpyDeviceToHost));
	return LS1HIP_OK;
}

extern "C" int ls1hip_planar_log(ls1hip_ctx* c, size_t cap_rows, double* rows2, size_t* nrows) {
	if (!c) return LS1HIP_EINVAL;
	const size_t have = c->d_pl_log ? std::min<size_t>(c->steplog_steps, STEPLOG_ROWS) : 0;
	if (nrows) *nrows = have;
	if (!rows2 || have == 0) return LS1HIP_OK;
	REQUIRE(c, cap_rows >= have, "buffer too small: %zu < %zu rows", cap_rows, have);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return ring_read(c, c->d_pl_log, 2 * sizeof(double), c->steplog_steps, STEPLOG_ROWS, rows2);
}
