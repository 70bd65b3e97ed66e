// api_rdf.hip — the C ABI of libls1hip (include/ls1hip.h), part 4: radial distribution functions sampled on the device
// (the reference's RDF plugin and RDFCellProcessor: io/RDF.{h,cpp}, particleContainer/adapter/RDFCellProcessor.cpp).
#include "api_internal.hpp"

static int rdf_nsites(const ls1hip_ctx* c, int k) { return c->h_ct.nlj[k] + c->h_ct.nc[k] + c->h_ct.nd[k] + c->h_ct.nq[k]; }

// words of the two histograms for the current component set: mol[p][bin], p over (i, j >= i) in the order of RDF::collectRDF
// (RDF.cpp:235-241); site blocks [m][n][bin] of the pairs with n_i + n_j > 2 (RDF.cpp:278-283) in the same order
static void rdf_words(const ls1hip_ctx* c, int bins, int site_rdf, size_t* mol, size_t* site, uint32_t* site_off) {
	const int nc = c->h_ct.ncomp;
	size_t mw = 0, sw = 0;
	int p = 0;
	for (int i = 0; i < nc; ++i)
		for (int j = i; j < nc; ++j, ++p) {
			mw += (size_t)bins;
			const int ni = rdf_nsites(c, i), nj = rdf_nsites(c, j);
			uint32_t off = 0xffffffffu;
			if (site_rdf && ni + nj > 2) {
				off = (uint32_t)sw;
				sw += (size_t)ni * nj * bins;
			}
			if (site_off) site_off[p] = off;
		}
	*mol = mw;
	*site = sw;
}

static void rdf_free(ls1hip_ctx* c) {
	dfree(c->d_rdf);
	c->rdf_bins = 0;
	c->rdf_site = 0;
	c->rdf_dr = 0.;
	c->rdf_mol_words = c->rdf_site_words = 0;
	c->rdf_samples = 0;
}

void rdf_destroy(ls1hip_ctx* c) {
	rdf_free(c);
	timer_free(c->t_rdf);
}

extern "C" int ls1hip_rdf_config(ls1hip_ctx* c, int bins, double interval_length, int site_rdf) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	if (bins == 0) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		rdf_free(c);
		return LS1HIP_OK;
	}
	REQUIRE(c, c->have_comp && c->have_domain, "ls1hip_rdf_config needs the components and the domain (ls1hip_set_components, ls1hip_set_domain)");
	REQUIRE(c, bins > 0, "bins must be > 0 (0 switches the sampling off), got %d", bins);
	REQUIRE(c, interval_length > 0., "interval_length must be > 0, got %g", interval_length);
	REQUIRE(c, std::isfinite(interval_length * bins) && std::isfinite(interval_length * interval_length * bins * bins),
			"bins * interval_length is not finite");
	size_t mw, sw;
	rdf_words(c, bins, site_rdf, &mw, &sw, nullptr);
	REQUIRE(c, mw + sw < (size_t)0x7fffffff, "histograms of %zu words exceed the 32-bit word index", mw + sw);
	HIPCHK(c, hipStreamSynchronize(c->stream));
	rdf_free(c);
	int rc = dalloc(c, &c->d_rdf, mw + sw + MAXC);
	if (rc) return rc;
	HIPCHK(c, hipMemsetAsync(c->d_rdf, 0, (mw + sw + MAXC) * sizeof(unsigned long long), c->stream));
	c->rdf_bins = bins;
	c->rdf_dr = interval_length;
	c->rdf_site = site_rdf ? 1 : 0;
	c->rdf_mol_words = mw;
	c->rdf_site_words = sw;
	return LS1HIP_OK;
}

extern "C" int ls1hip_rdf_layout(const ls1hip_ctx* c, size_t* mol_words, size_t* site_words) {
	if (!c) return LS1HIP_EINVAL;
	if (mol_words) *mol_words = c->rdf_mol_words;
	if (site_words) *site_words = c->rdf_site_words;
	return LS1HIP_OK;
}

// one traversal over the current positions; the caller has checked nothing
int rdf_sample_impl(ls1hip_ctx* c) {
	REQUIRE(c, c->rdf_bins > 0 && c->d_rdf, "RDF sampling is not configured (ls1hip_rdf_config)");
	// between two builds of the neighbour lists a drift leaves the binning of the last build in place (stale by at most skin / 2, the
	// grid is sized by r_c + skin): that is what the list force pass walks too.  On multi-rank domains a re-binning in progress
	// (ls1hip_rebin before import_done(0)) keeps the lists formally alive, so only a finished binning counts there.
	REQUIRE(c, c->binned || (c->vl_ready && !c->has_remote), "molecules are not binned (call ls1hip_rebin)");
	REQUIRE(c, c->halo_valid, "halo not populated (call ls1hip_halo / import_done(1), or ls1hip_halo_refresh between list builds)");
	REQUIRE(c, !c->fused_split && !c->inner_in_flight, "a split force pass is in flight");
	REQUIRE(c, c->g.hw == 1, "RDF sampling serves grids with one cell per cutoff (cells_in_cutoff = 1)");
	RdfParams R;
	memset(&R, 0, sizeof(R));
	size_t mw, sw;
	rdf_words(c, c->rdf_bins, c->rdf_site, &mw, &sw, R.site_off);
	REQUIRE(c, mw == c->rdf_mol_words && sw == c->rdf_site_words, "the component set changed since ls1hip_rdf_config");
	const MolSoA& m = c->mol[c->cur];
	// pos_x may also name the force arrays (after a fused per-step pass), but then the molecules are not binned: refused above
	ForceParams P;
	memset(&P, 0, sizeof(P));
	P.g = c->g;
	P.x = c->pos_x ? c->pos_x : m.x; P.y = c->pos_x ? c->pos_y : m.y; P.z = c->pos_x ? c->pos_z : m.z;
	P.q0 = m.q0; P.q1 = m.q1; P.q2 = m.q2; P.q3 = m.q3;
	P.cid = m.cid;
	P.cell_begin = c->d_cell_begin; P.cell_end = c->d_cell_end;
	P.ct = c->d_ct;
	P.cnt = c->d_cnt;
	R.bins = c->rdf_bins;
	R.ncomp = c->h_ct.ncomp;
	R.dr = c->rdf_dr;
	R.maxd2 = c->rdf_dr * c->rdf_dr * (double)c->rdf_bins * (double)c->rdf_bins;  // RDF.cpp:47, same order of the products
	R.rc2 = c->rc * c->rc;                                                        // RDFCellProcessor.h: cutoffRadius * cutoffRadius
	for (int k = 0; k < R.ncomp; ++k) R.nsites[k] = rdf_nsites(c, k);
	R.mol_words = (uint32_t)mw;
	R.site_words = (uint32_t)sw;
	R.id = m.id;
	R.hsrc = c->d_halo_src;
	R.g_mol = c->d_rdf;
	R.g_site = c->d_rdf + mw;
	R.g_n = c->d_rdf + mw + sw;
	const double ncell = (double)c->g.box[0] * c->g.box[1] * c->g.box[2];
	{
		TimedScope ts(c, c->t_rdf);
		if (!launch_rdf(P, R, c->h_ct.has_rot != 0, ncell > 0 ? (double)c->n_real / ncell : 0., c->stream))
			FAIL(c, LS1HIP_EINVAL, "the RDF pass could not be launched for this grid");
	}
	HIPCHK(c, hipGetLastError());
	c->rdf_samples++;  // RDF::tickRDF
	return LS1HIP_OK;
}

extern "C" int ls1hip_rdf_sample(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	return rdf_sample_impl(c);
}

extern "C" int ls1hip_rdf_read(ls1hip_ctx* c, uint64_t* mol, size_t cap_mol, uint64_t* site, size_t cap_site, uint64_t* n_per_component,
							   uint64_t* samples) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, c->rdf_bins > 0 && c->d_rdf, "RDF sampling is not configured (ls1hip_rdf_config)");
	REQUIRE(c, !mol || cap_mol >= c->rdf_mol_words, "molecule histogram buffer too small: %zu < %zu words", cap_mol, c->rdf_mol_words);
	REQUIRE(c, !site || cap_site >= c->rdf_site_words, "site histogram buffer too small: %zu < %zu words", cap_site, c->rdf_site_words);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	const size_t mw = c->rdf_mol_words, sw = c->rdf_site_words;
	if (mol && mw) HIPCHK(c, hipMemcpy(mol, c->d_rdf, mw * sizeof(uint64_t), hipMemcpyDeviceToHost));
	if (site && sw) HIPCHK(c, hipMemcpy(site, c->d_rdf + mw, sw * sizeof(uint64_t), hipMemcpyDeviceToHost));
	if (n_per_component) HIPCHK(c, hipMemcpy(n_per_component, c->d_rdf + mw + sw, (size_t)c->h_ct.ncomp * sizeof(uint64_t), hipMemcpyDeviceToHost));
	if (samples) *samples = c->rdf_samples;
	return LS1HIP_OK;
}

extern "C" int ls1hip_rdf_reset(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, c->rdf_bins > 0 && c->d_rdf, "RDF sampling is not configured (ls1hip_rdf_config)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemsetAsync(c->d_rdf, 0, (c->rdf_mol_words + c->rdf_site_words + MAXC) * sizeof(unsigned long long), c->stream));
	c->rdf_samples = 0;
	return LS1HIP_OK;
}
