// api_odf.hip — the C ABI of libls1hip (include/ls1hip.h), part 9: orientation distribution functions sampled on the device
// (the reference's ODF plugin and ODFCellProcessor: io/ODF.{h,cpp}, particleContainer/adapter/ODFCellProcessor.cpp).
#include "api_internal.hpp"

// bit c: component c has exactly one dipole (ODFCellProcessor.cpp:25,34; ODF::init, ODF.cpp:37-48)
static uint32_t odf_dipole_mask(const ls1hip_ctx* c) {
	uint32_t m = 0;
	for (int k = 0; k < c->h_ct.ncomp; ++k)
		if (c->h_ct.nd[k] == 1) m |= 1u << k;
	return m;
}

static void odf_free(ls1hip_ctx* c) {
	dfree(c->d_odf);
	c->odf_phi = c->odf_gamma = 0;
	c->odf_shell = 0.;
	c->odf_mask = 0;
	c->odf_words = 0;
	c->odf_samples = 0;
}

void odf_destroy(ls1hip_ctx* c) { odf_free(c); }

// ODF::readXML + ODF::init (ODF.cpp:6-79)
extern "C" int ls1hip_odf_config(ls1hip_ctx* c, int phi1_increments, int phi2_increments, int gamma_increments, double shell_cutoff) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	if (phi1_increments == 0 && phi2_increments == 0 && gamma_increments == 0) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		odf_free(c);
		return LS1HIP_OK;
	}
	REQUIRE(c, c->have_comp && c->have_domain, "ls1hip_odf_config needs the components and the domain (ls1hip_set_components, ls1hip_set_domain)");
	REQUIRE(c, phi1_increments > 0 && phi2_increments > 0 && gamma_increments > 0,
			"increments must be > 0 (all three 0 switch the sampling off), got %d %d %d", phi1_increments, phi2_increments, gamma_increments);
	// elementIDreversed = indexPhi2 * _phi2Increments * _gammaIncrements + ... (ODF.cpp:306) is the transposed index only for equal
	// increments; with phi1 < phi2 it can lie behind the reference's arrays
	REQUIRE(c, phi1_increments == phi2_increments, "phi1_increments != phi2_increments (%d, %d) is not served: the reference's reversed element index is ill-defined there",
			phi1_increments, phi2_increments);
	REQUIRE(c, shell_cutoff > 0. && shell_cutoff <= c->rc, "shell_cutoff must lie in (0, r_c = %g], got %g", c->rc, shell_cutoff);
	const uint32_t mask = odf_dipole_mask(c);
	// the reference keeps four arrays, keyed by the component ids 0 and 1 (ODF.cpp:311-329; more pairings: its error at :73-76)
	REQUIRE(c, (mask & ~3u) == 0, "a component with id >= 2 has exactly one dipole: the ODF has the reference's four arrays of the ids 0 and 1 only");
	const size_t W = (size_t)phi1_increments * phi2_increments * gamma_increments + 1;  // _numElements, ODF.cpp:51
	REQUIRE(c, 4 * W < (size_t)0x7fffffff, "four arrays of %zu words exceed the 32-bit word index", W);
	HIPCHK(c, hipStreamSynchronize(c->stream));
	odf_free(c);
	int rc = dalloc(c, &c->d_odf, 4 * W);
	if (rc) return rc;
	HIPCHK(c, hipMemsetAsync(c->d_odf, 0, 4 * W * sizeof(unsigned long long), c->stream));
	c->odf_phi = phi1_increments;
	c->odf_gamma = gamma_increments;
	c->odf_shell = shell_cutoff;
	c->odf_mask = mask;
	c->odf_words = W;
	return LS1HIP_OK;
}

extern "C" int ls1hip_odf_layout(const ls1hip_ctx* c, size_t* words_per_array) {
	if (!c) return LS1HIP_EINVAL;
	if (words_per_array) *words_per_array = c->odf_words;
	return LS1HIP_OK;
}

// one traversal over the current positions and orientations (ODF::afterForces -> traverseCells(ODFCellProcessor), ODF.cpp:81-85)
int odf_sample_impl(ls1hip_ctx* c) {
	REQUIRE(c, c->odf_phi > 0 && c->d_odf, "ODF sampling is not configured (ls1hip_odf_config)");
	if (int rc = sample_gate(c)) return rc;
	REQUIRE(c, c->g.hw == 1, "ODF sampling serves grids with one cell per cutoff (cells_in_cutoff = 1)");
	REQUIRE(c, odf_dipole_mask(c) == c->odf_mask, "the component set changed since ls1hip_odf_config");
	const MolSoA& m = c->mol[c->cur];
	ForceParams P;
	memset(&P, 0, sizeof(P));
	fill_cell_args(c, P);
	OdfParams O;
	memset(&O, 0, sizeof(O));
	O.P = c->odf_phi;
	O.G = c->odf_gamma;
	O.W = (uint32_t)c->odf_words;
	O.cut2 = std::min(c->rc * c->rc, c->odf_shell * c->odf_shell);  // ODFCellProcessor.cpp:40 and ODF.cpp:151
	O.dip_mask = c->odf_mask;
	O.id = m.id;
	O.hsrc = c->d_halo_src;
	O.g_hist = c->d_odf;
	{
		TimedScope ts(c, c->t_odf);
		if (!launch_odf(P, O, c->h_ct.has_rot != 0, mean_per_cell(c), c->stream))
			FAIL(c, LS1HIP_EINVAL, "the ODF pass could not be launched for this grid");
	}
	HIPCHK(c, hipGetLastError());
	c->odf_samples++;
	return LS1HIP_OK;
}

extern "C" int ls1hip_odf_sample(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	return odf_sample_impl(c);
}

// the local arrays ODF::collect sums over the ranks (ODF.cpp:333-384)
extern "C" int ls1hip_odf_read(ls1hip_ctx* c, uint64_t* hist, size_t cap, uint64_t* samples) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, c->odf_phi > 0 && c->d_odf, "ODF sampling is not configured (ls1hip_odf_config)");
	REQUIRE(c, !hist || cap >= 4 * c->odf_words, "histogram buffer too small: %zu < %zu words", cap, 4 * c->odf_words);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (hist) HIPCHK(c, hipMemcpy(hist, c->d_odf, 4 * c->odf_words * sizeof(uint64_t), hipMemcpyDeviceToHost));
	if (samples) *samples = c->odf_samples;
	return LS1HIP_OK;
}

// ODF::reset (ODF.cpp:104-121)
extern "C" int ls1hip_odf_reset(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, c->odf_phi > 0 && c->d_odf, "ODF sampling is not configured (ls1hip_odf_config)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemsetAsync(c->d_odf, 0, 4 * c->odf_words * sizeof(unsigned long long), c->stream));
	c->odf_samples = 0;
	return LS1HIP_OK;
}
