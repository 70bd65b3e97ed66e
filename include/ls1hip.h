/*
 * ls1hip.h — C ABI of libls1hip, the MI355X-native linked-cell pair-force engine.
 *
 * This is the drop-in boundary for ONE hot path of ls1-MarDyn (reference: reinago/ls1-mardyn):
 *   LinkedCells traversal -> VectorizedCellProcessor pair kernel -> Leapfrog integrator (+ ghost-cell halo).
 * Every entry point names the reference interface it replaces (paths relative to /root/reference/src).
 * Host adapters (C++17 classes with the reference's ParticleContainer / CellProcessor / Integrator signatures,
 * or the Python mirror in ls1-mardyn_amd/) call ONLY these functions.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, FP64 only (the reference's MARDYN_DPDP build).
 *   - every function returns 0 on success, <0 on error (LS1HIP_E*); ls1hip_last_error() gives the text.
 *     (reference convention: log + Simulation::exit(code), Simulation.cpp:155-158 — adapters translate.)
 *   - the caller owns every host buffer; the library owns device memory and HIP streams; no pointer passed in
 *     is retained after the call returns.  `dev_*` arguments are DEVICE pointers (e.g. torch tensor data_ptr()).
 *   - entry points are main-thread only and internally asynchronous on the context's HIP streams
 *     (reference threading contract: SURVEY.md 8b).
 *   - molecule arrays are AoS [n][k] row-major exactly like the reference's Molecule fields:
 *     r[3], v[3], q[4]=(w,x,y,z), D[3] (angular momentum), F[3], M[3], Vi[3]; cid is 0-based.
 */
#ifndef LS1HIP_H_
#define LS1HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ls1hip_ctx ls1hip_ctx;

enum {
	LS1HIP_OK = 0,
	LS1HIP_EINVAL = -1,   /* bad argument / call order                                   */
	LS1HIP_EHIP = -2,     /* HIP runtime error                                           */
	LS1HIP_ENOMEM = -3,   /* device allocation failed / capacity exceeded                */
	LS1HIP_ELOST = -4,    /* a molecule left the halo region (reference: "particle lost")*/
	LS1HIP_ENODEV = -5    /* no usable gfx950 device                                     */
};

/* site table strides (doubles per site), same column order as the reference's .inp component block
 * (io/ASCIIReader.cpp:178-206) with the LJ shift already reduced to shift6 (molecules/Component.cpp:105-118) */
#define LS1HIP_LJ_STRIDE 7 /* x y z m eps sigma shift6 */
#define LS1HIP_CH_STRIDE 5 /* x y z m q                */
#define LS1HIP_DP_STRIDE 7 /* x y z ex ey ez absMy     */
#define LS1HIP_QP_STRIDE 7 /* x y z ex ey ez absQ      */

/* force-kernel variants (ls1hip_set_option "force_kernel") */
#define LS1HIP_FK_AUTO 0      /* fastest parity-green kernel for the component set           */
#define LS1HIP_FK_GENERIC 1   /* thread-per-molecule, global-memory neighbours (any density) */
#define LS1HIP_FK_LDS_LIST 2  /* brick-tiled, LDS-staged, per-lane neighbour lists (1CLJ)    */
#define LS1HIP_FK_MS_BRICK 3  /* multi-site, LDS-staged molecule pairs; bitwise == GENERIC (AUTO's choice for multi-site sets) */
#define LS1HIP_FK_MS_SITES 4  /* multi-site, LDS tables + cached own sites + FMA bodies; 1e-12 of GENERIC; on request only   */
#define LS1HIP_FK_NEIGHBOUR_LIST 5 /* reported by "last_force_kernel" only: forces from the stored neighbour lists (ls1hip_set_verlet) */

/* ---- lifetime ------------------------------------------------------------------------------------------------- */

/* Create a context on HIP device `device` (one process per GPU; multi-GPU = one context per rank).
 * Replaces: construction of LinkedCells + VectorizedCellProcessor + Leapfrog in Simulation::readXML /
 * prepare_start (Simulation.cpp:411-455, 768-779, 168-186). */
int ls1hip_create(int device, ls1hip_ctx** out);
int ls1hip_destroy(ls1hip_ctx* ctx);
/* Text of the last error on this context (never NULL).  ctx may be NULL for creation errors. */
const char* ls1hip_last_error(const ls1hip_ctx* ctx);
/* Library version / build target string, e.g. "ls1hip 0.1 gfx950" ("... +variant": see option "build_variant"). */
const char* ls1hip_version(void);

/* Integer options: "force_kernel" (LS1HIP_FK_*), "cells_in_cutoff" (1|2, LinkedCells <cellsInCutoffRadius>,
 * particleContainer/LinkedCells.h:81-106), "compute_vi" (0|1 per-molecule virial Vi output),
 * "deterministic" (0|1 canonical in-cell order by molecule id),
 * "count_pairs" (0|1 tally molecule pairs / site interactions inside the cutoff for ls1hip_pair_stats — the
 * counters of adapter/FlopCounter.cpp:20-76; forces then use the generic kernel),
 * "build_variant" (read only: 0 = the regular library; 1 = the library contains an object built by tools/ab_variant.sh as a
 *   timing / layout variant of a kernel — such builds may compute WRONG forces by construction and are for same-box A/B timing only;
 *   ls1hip_version() then ends in "+variant"),
 * "last_force_kernel" (read only: kernel family of the last force launch — LS1HIP_FK_*: 1 generic, 2 single-centre LJ brick
 *   kernels, 3 multi-site brick kernel, 4 multi-site site kernel, 5 neighbour-list force pass; lets callers / tests see a fallback to the generic kernel),
 * "precision" (list force pass of the single-centre LJ path: 0 = FP64 (default), 1 = SPDP, 2 = SPSP — the reference's
 *   MARDYN_SPDP / MARDYN_SPSP build modes, vectorization/RealVec.h, RealAccumVecSPDP.h: pair arithmetic in FP32, sums in
 *   FP64 / FP32; molecule state, integration and reductions stay FP64; used while every brick of the last list build is
 *   regular, read-only "precision_in_use" tells),
 * "local_rebuild" (neighbour-list loop of a single periodic domain, fused passes: 1 (default) = the lists are rebuilt when
 * the pair-displacement bound of some brick neighbourhood exceeds skin / 2 — sum over the steps of dt * (s1 + s2) / 2, s1 >= s2
 * the two largest speeds among the molecules of the 27 bricks around a brick; 0 = global bound, sum of dt * v_max; both are
 * rigorous, the local one is never earlier),
 * "overlap_halo" (ls1hip_run: 0 = halo, then one traversal of all cells (default, fastest on a single GPU); 1 = inner
 *   cells first, the halo built on a second stream meanwhile, then the boundary cells — the order a transport-driven
 *   multi-rank loop uses; 2 = halo, inner cells, boundary cells on one stream),
 * "fuse_integration" (0|1, default 1: ls1hip_run lets the force pass do the integration between steps, see
 * ls1hip_forces_kick_drift), "can_fuse_integration" (read only), "can_fuse_rigid_lists" (read only: a single-component
 *   rigid multi-site set under neighbour lists — ls1hip_run lets the pair-stream list pass integrate its own molecules,
 *   ls1hip_forces_list with dt > 0 does it piecewise; bitwise the separate kick + kick + drift pass),
 * "lj_split" (variant of the single-centre LJ fast path; results are the same to rounding, only speed differs:
 *   0 = choose from the mean cell occupancy (default); 1 | 2 = list kernel with 1 | 2 lanes per molecule;
 *   4 = FP32 MFMA distance-tile pre-filter + exact FP64 evaluation, 1x4x4-cell bricks, 512 threads;
 *   5 = the same with 256 threads (larger staging area); 6 = 1x4x2-cell bricks (dense cells).
 *   4-6 need cells_in_cutoff = 1 and fall back to the list kernel otherwise). */
int ls1hip_set_option(ls1hip_ctx* ctx, const char* name, long value);
int ls1hip_get_option(const ls1hip_ctx* ctx, const char* name, long* value);

/* ---- model ---------------------------------------------------------------------------------------------------- */

/* Component set + cutoffs -> device parameter tables.
 * Replaces: Comp2Param::initialize (molecules/Comp2Param.cpp:10-187), the table build in
 * VectorizedCellProcessor::VectorizedCellProcessor (adapter/VectorizedCellProcessor.cpp:21-83) and
 * Ensemble::setComponentLookUpIDs (ensemble/EnsembleBase.cpp:88-101).
 * nlj/nc/nd/nq: [ncomp] site counts; lj/ch/dp/qp: flat site tables (component-major, strides above);
 * mass: [ncomp]; I: [ncomp][3] principal moments; mix: [ncomp*(ncomp-1)/2][2] = (xi, eta) for i<j in reader
 * order (io/ASCIIReader.cpp:221-230); eps_rf: reaction-field epsilon; rc / rc_lj: cutoffs. */
int ls1hip_set_components(ls1hip_ctx* ctx, int ncomp, const int* nlj, const int* nc, const int* nd, const int* nq,
						  const double* lj, const double* ch, const double* dp, const double* qp, const double* mass,
						  const double* I, const double* mix, double eps_rf, double rc, double rc_lj);

/* Rotational degrees of freedom per component as the reference counts them: Component::getRotationalDegreesOfFreedom
 * (molecules/Component.cpp:140-167 — from the moments of the SITE masses; the I line of an .inp, io/ASCIIReader.cpp:208-212, or
 * <momentsofinertia>, Component.cpp:88-97, may override the VALUES of the moments afterwards without changing this count).
 * Optional: ls1hip_set_components derives the count of non-zero moments of `I`, which is the same number unless such an override
 * turned a zero moment into a non-zero one.  Only the thermostat's degree-of-freedom sums use it (integrators/Leapfrog.cpp:100,126
 * -> Domain.cpp:204-240), never the motion.  Call after ls1hip_set_components. */
int ls1hip_set_rot_dof(ls1hip_ctx* ctx, int ncomp, const int* rot_dof);

/* Read back the derived LJ table ([ncenters][ncenters] each; ncenters = sum nlj) — for parity tests of the
 * parameter derivation.  Any pointer may be NULL. */
int ls1hip_get_lj_table(const ls1hip_ctx* ctx, int* ncenters, double* eps24, double* sig2, double* shift6);

/* Domain of THIS rank: bounding box [box_min, box_max) inside the global periodic box of edge global_len
 * (origin 0).  neighbor_rank[27]: rank owning the region in direction (sx,sy,sz) in {-1,0,1}^3, index
 * (sz+1)*9+(sy+1)*3+(sx+1); an entry equal to `my_rank` means "periodic image handled locally", -1 means
 * open boundary (no halo from that side).  For a single GPU pass all entries = my_rank (periodic) or -1 (open).
 * Replaces: LinkedCells::LinkedCells / rebuild (particleContainer/LinkedCells.cpp:42-109,136-204),
 * DomainDecompBase::getBoundingBoxMin/Max and DomainDecomposition grid setup
 * (parallel/DomainDecomposition.cpp:19-41,112-123). */
int ls1hip_set_domain(ls1hip_ctx* ctx, const double global_len[3], const double box_min[3], const double box_max[3],
					  int my_rank, const int neighbor_rank[27]);
/* Cell grid chosen for the domain: dims[3] incl. halo layers, cell_len[3]. */
int ls1hip_get_grid(const ls1hip_ctx* ctx, int dims[3], double cell_len[3], int* halo_width);

/* ---- molecules ------------------------------------------------------------------------------------------------ */

/* Replace the molecule set of this rank (all must lie inside [box_min, box_max)).
 * Replaces: ParticleContainer::addParticles (particleContainer/ParticleContainer.h:108-130).
 * q and D may be NULL (unit quaternion / zero angular momentum). */
int ls1hip_upload(ls1hip_ctx* ctx, size_t n, const uint64_t* id, const int32_t* cid, const double* r, const double* v,
				  const double* q, const double* D);
/* Streaming form of ls1hip_upload for phase spaces that should never exist twice on the host (the 10^8 restart case,
 * SURVEY.md 8f-3): announce an upper bound of the total (it sizes the device arrays), hand over any number of chunks,
 * finish; the molecules actually handed over become the molecule set.  Chunks are copied raw to the device
 * and transposed into the device SoA there (no host-side Molecule objects, no host-side SoA copies).
 * ls1hip_upload_records takes the records of the reference's binary checkpoint as they lie in the file:
 *   LS1HIP_REC_ICRVQD 116 B {id u64, cid u32 (1-based), r 3 f64, v 3 f64, q 4 f64, D 3 f64}
 *                     (FullMolecule::writeBinary, molecules/FullMolecule.cpp:451-473; Domain.cpp:572-595),
 *   LS1HIP_REC_ICRV    60 B {id, cid, r, v},  LS1HIP_REC_IRV 56 B {id, r, v}   (io/BinaryReader.cpp:103-108,179-213;
 *                     q = (1,0,0,0), D = 0, and cid = 1 for IRV).
 * Replaces: BinaryReader::readPhaseSpace -> ParticleContainer::addParticle (io/BinaryReader.cpp:140-260).
 * Errors (molecule outside the bounding box, wrong component id) are reported by ls1hip_upload_end. */
#define LS1HIP_REC_ICRVQD 0
#define LS1HIP_REC_ICRV 1
#define LS1HIP_REC_IRV 2
int ls1hip_upload_begin(ls1hip_ctx* ctx, size_t n_total);
int ls1hip_upload_chunk(ls1hip_ctx* ctx, size_t n, const uint64_t* id, const int32_t* cid, const double* r,
						const double* v, const double* q, const double* D);
int ls1hip_upload_records(ls1hip_ctx* ctx, size_t n, const void* records, int format);
/* ls1hip_upload_chunk for producers that already live on the GPU (generators, RCCL receive buffers): the arrays are
 * DEVICE pointers on the context's device, complete when the call is made (synchronise the producing stream first);
 * they may be released when the call returns. */
int ls1hip_upload_chunk_device(ls1hip_ctx* ctx, size_t n, const uint64_t* dev_id, const int32_t* dev_cid,
							   const double* dev_r, const double* dev_v, const double* dev_q, const double* dev_D);
int ls1hip_upload_end(ls1hip_ctx* ctx);
/* Owned molecules [first, first + n) in device order as ICRVQD records (the payload of the reference's binary
 * checkpoint, written by ParticleContainer iteration + FullMolecule::writeBinary in io/CheckpointWriter /
 * Domain::writeCheckpoint, Domain.cpp:572-595); positions are wrapped into the box. */
int ls1hip_download_records(ls1hip_ctx* ctx, size_t first, size_t n, void* records);

/* Number of molecules owned by this rank / halo copies currently held. */
int ls1hip_count(const ls1hip_ctx* ctx, size_t* n_owned, size_t* n_halo);

/* Download owned molecules in device (cell-sorted) order.  Any pointer may be NULL.
 * Replaces: ParticleContainer::iterator(ONLY_INNER_AND_BOUNDARY) read access (ParticleContainer.h:150-170). */
int ls1hip_download_state(ls1hip_ctx* ctx, size_t cap, uint64_t* id, int32_t* cid, double* r, double* v, double* q,
						  double* D);
/* Forces of the last ls1hip_forces call, same order as ls1hip_download_state.
 * Replaces: Molecule::F / M / Vi after Simulation::updateForces -> calcFM (Simulation.cpp:752-762). */
int ls1hip_download_forces(ls1hip_ctx* ctx, size_t cap, double* F, double* M, double* Vi);

/* ---- the time step, piecewise (mirrors Simulation::simulate, Simulation.cpp:995-1099) ----------------------- */

/* Leapfrog::eventNewTimestep -> FullMolecule::upd_preF (integrators/Leapfrog.cpp:48-64,
 * molecules/FullMolecule.cpp:334-364): v += dt/2m F; r += dt v; quaternion / L half steps. */
int ls1hip_kick_drift(ls1hip_ctx* ctx, double dt);
/* ls1hip_scale_velocities(beta_trans, beta_rot) followed by ls1hip_kick_drift(dt) in ONE pass over the molecules (what
 * Simulation::simulate does between two steps of an NVT run: VelocityScalingThermostat::apply, Simulation.cpp:1108-1131, then
 * Integrator::eventNewTimestep); the arithmetic is that of the two separate calls, operation for operation. */
int ls1hip_scale_kick_drift(ls1hip_ctx* ctx, double beta_trans, double beta_rot, double dt);

/* LinkedCells::update (LinkedCells.cpp:243-356): re-sort owned molecules into cells; molecules that left the box
 * through a side whose neighbor_rank is this rank are wrapped (DomainDecompBase::handleDomainLeavingParticles,
 * parallel/DomainDecompBase.cpp:174-225); molecules leaving towards other ranks are packed for export
 * (see ls1hip_export_*). */
int ls1hip_rebin(ls1hip_ctx* ctx);

/* Halo population for all directions handled locally (DomainDecompBase::populateHaloLayerWithCopies,
 * parallel/DomainDecompBase.cpp:293-348) and packing of halo copies for remote directions; then
 * LinkedCells::updateMoleculeCaches (LinkedCells.cpp:1054-1086: site expansion, F/M/Vi cleared). */
int ls1hip_halo(ls1hip_ctx* ctx);

/* LinkedCells::traverseCells(VectorizedCellProcessor) + Simulation::updateForces (LinkedCells.cpp:564-575,
 * VectorizedCellProcessor.cpp:111-157,796-2821; FullMolecule::calcFM molecules/FullMolecule.cpp:526-629).
 * upot / virial = the values the reference passes to Domain::setLocalUpot / setLocalVirial
 * (VectorizedCellProcessor.cpp:155-156) for THIS rank; each pair that crosses a rank/periodic boundary is
 * counted half on each side, so the sum over ranks equals the reference's global value.
 * which: 0 = all cells, 1 = inner cells only (no halo cell in the neighbourhood;
 * LinkedCells::traversePartialInnermostCells), 2 = the remaining (boundary) cells
 * (LinkedCells::traverseNonInnermostCells) — the reference's comm/compute overlap split
 * (parallel/NonBlockingMPIMultiStepHandler.cpp:30-97).  Results of 1 then 2 accumulate. */
int ls1hip_forces(ls1hip_ctx* ctx, int which, double* upot, double* virial);

/* Leapfrog::eventForcesCalculated -> FullMolecule::upd_postF (Leapfrog.cpp:66-150, FullMolecule.cpp:366-389):
 * v += dt_half/m F; L += dt_half M; returns sum m v^2, sum I w^2, N, rotational DOF (thermostat 0). */
int ls1hip_kick(ls1hip_ctx* ctx, double dt_half, double* summv2, double* sumIw2, uint64_t* n, uint64_t* rot_dof);
/* The kinetic sums of the last ls1hip_kick, for callers that queued it with NULL outputs (asynchronously) and fetch later. */
int ls1hip_kinetic_sums(ls1hip_ctx* ctx, double* summv2, double* sumIw2, uint64_t* n, uint64_t* rot_dof);
/* Component-wise thermostats (Domain::severalThermostats()): the sums of Leapfrog::transition2to3 (integrators/Leapfrog.cpp:84-104)
 * per COMPONENT — arrays of ncomp entries: sum m v^2, sum I w^2, N, rotational DOF of the component's owned molecules, from the
 * current velocities (call after ls1hip_kick).  The caller folds components into thermostats (Domain::getThermostat). */
int ls1hip_kinetic_sums_by_component(ls1hip_ctx* ctx, int ncomp, double* summv2, double* sumIw2, uint64_t* n, uint64_t* rot_dof);
/* Overlap of host and device work around a traversal: ls1hip_forces / ls1hip_forces_list with upot = virial = NULL only queue
 * the kernels.  ls1hip_traversal_mark queues a copy of the traversal's sums behind them; ls1hip_traversal_sums waits for THAT
 * copy only — whatever was queued after the mark (typically the post-force ls1hip_kick with NULL outputs) keeps running on
 * the device while the host goes on with U_pot and the virial (what VectorizedCellProcessor::endTraversal publishes). */
int ls1hip_traversal_mark(ls1hip_ctx* ctx);
int ls1hip_traversal_sums(ls1hip_ctx* ctx, double* upot, double* virial);

/* Force pass that consumes the forces at once (reduced-memory mode; the reference's counterpart is the RMM pair
 * VCP1CLJRMM::processCell* + LeapfrogRMM, particleContainer/adapter/VCP1CLJRMM.cpp:241-369, integrators/LeapfrogRMM.cpp):
 * ls1hip_forces(which) fused with the post-force kick of this step and the pre-force kick + drift of the NEXT step,
 * arithmetic identical to ls1hip_forces + ls1hip_kick_then_kick_drift(dt) (bitwise).  F is never stored (-48 B of
 * HBM traffic per molecule, no separate integrator pass); the advanced positions are picked up by the following
 * ls1hip_rebin.  Afterwards velocities are at the half step, forces are NOT available (ls1hip_download_forces fails
 * until the next ls1hip_forces).  which = 0, or 1 followed by 2 (overlap split), as for ls1hip_forces; U_pot / virial
 * as there.  Available when ls1hip_get_option("can_fuse_integration") is 1: single-centre LJ fast path, no per-molecule
 * virial, no device thermostat.  ls1hip_run uses it between steps unless option "fuse_integration" is 0. */
int ls1hip_forces_kick_drift(ls1hip_ctx* ctx, int which, double dt, double* upot, double* virial);

/* eventForcesCalculated of step n immediately followed by eventNewTimestep of step n+1 (Leapfrog.cpp:66-150 then
 * :48-64) in ONE pass over the molecules: v += dt/m F; r += dt v (and the rotational counterparts) — bitwise the same
 * as ls1hip_kick(dt/2) + ls1hip_kick_drift(dt), for steps whose kinetic sums are not needed (NVE, no output). */
int ls1hip_kick_then_kick_drift(ls1hip_ctx* ctx, double dt);
/* ls1hip_scale_kick_drift with one factor pair per COMPONENT: VelocityScalingThermostat::apply, componentwise branch
 * (thermostats/VelocityScalingThermostat.cpp:45-69; the driver sets the factors of a component's thermostat,
 * Simulation.cpp:1111-1127), folded into the pre-force kick + drift pass. */
int ls1hip_scale_kick_drift_components(ls1hip_ctx* ctx, int ncomp, const double* beta_trans, const double* beta_rot, double dt);

/* VelocityScalingThermostat::apply, global branch (thermostats/VelocityScalingThermostat.cpp:80-96): v *= beta_trans,
 * D *= beta_rot for every owned molecule. */
int ls1hip_scale_velocities(ls1hip_ctx* ctx, double beta_trans, double beta_rot);

/* Global velocity-scaling thermostat inside ls1hip_run: after every post-force kick the device computes
 * beta_trans = (3 N T / sum m v^2)^0.4, beta_rot = (rotDOF T / sum I w^2)^0.4 exactly as Domain::calculateGlobalValues
 * does for thermostat 0 (Domain.cpp:204-240) and applies them, without a host round trip.  enabled = 0 -> NVE.
 * (Single-rank domains; multi-rank hosts reduce the sums and call ls1hip_scale_velocities.) */
int ls1hip_set_thermostat(ls1hip_ctx* ctx, int enabled, double target_temperature);

/* Homogeneous long-range correction: the constants Homogeneous::init / calculateLongRange compute and
 * hand to Domain::setUpotCorr / setVirialCorr (longRange/Homogeneous.cpp:21-135; LJ tail integrals of Lustig 1988,
 * :137-180; dipole reaction-field self term).  Host arithmetic on the component tables of this context.
 * n_per_component[ncomp]: global molecule count per component; global_rho = N / V. */
int ls1hip_long_range_homogeneous(ls1hip_ctx* ctx, const uint64_t* n_per_component, double global_rho,
								  double* upot_corr, double* virial_corr);

/* Neighbour-list reuse for ls1hip_run (single-centre LJ fast path, single rank, one cell per cutoff): the cell grid, the
 * halo shell and per-molecule neighbour lists are built with rc + skin and kept for as many steps as no molecule can have
 * moved by more than skin / 2 — the fused force pass reports max |v| of every step, the device accumulates the
 * displacement bound sum(dt * vmax) and ls1hip_run re-bins / rebuilds exactly when it exceeds skin / 2 (no guessed
 * interval; forces, U_pot and virial are the per-step kernels' to rounding, every listed pair is re-tested against rc in
 * FP64).  Between rebuilds there is no search, no re-binning and no halo regeneration.  Must be called after
 * ls1hip_set_components and before ls1hip_set_domain.  Positions reported by the download calls are wrapped into the box.
 * Precedent in the reference: the Verlet-list containers behind particleContainer/AutoPasContainer.cpp:281-346
 * (verletSkinRadius / verletRebuildFrequency).  enabled = 1: used when the mean population of a brick's region fits the
 * LDS staging area of the list kernels (otherwise ls1hip_run keeps the per-step kernels); 2: always (bricks that do not fit
 * are evaluated from global memory: correct, slow — for tests).  Read-only options "verlet_lists", "verlet_builds", "verlet_steps",
 * "verlet_ready" (lists built and alive), "verlet_bound_pending" (a drift since the lists were built / last polled: ls1hip_verlet_poll
 * may be asked), "verlet_irregular_bricks", "list_kick_available" (ls1hip_forces_list_kick applies). */
int ls1hip_set_verlet(ls1hip_ctx* ctx, int enabled, double skin);

/* The list mode piecewise — what a transport-driven multi-rank loop calls between two rebuilds (ls1hip_run is the
 * single-rank loop built from the same pieces).  Between rebuilds no molecule changes its owner (it may sit up to
 * skin / 2 outside its rank's box) and every halo copy keeps its slot; per step only POSITIONS travel:
 *   rebuild step:  ls1hip_rebin -> leaving exchange -> ls1hip_halo -> halo exchange (kind 1) -> ls1hip_verlet_build
 *                  -> ls1hip_forces_list
 *   reuse step:    ls1hip_forces_list(which=1) [inner bricks, needs owned positions only] || ls1hip_halo_refresh ->
 *                  refresh exchange (kind 2: LS1HIP_REFRESH_DOUBLES = 3 doubles per record, the records of the build-time
 *                  halo exchange in the same order and number: no count exchange) -> ls1hip_forces_list(which=2)
 * ls1hip_forces_list: dt > 0 fuses the pass with the integration (as ls1hip_forces_kick_drift), dt = 0 leaves F.
 * ls1hip_verlet_poll: after a fused pass — has this rank's displacement bound exceeded skin / 2?  The ranks must agree on
 * a rebuild (reduce the flags with a maximum).
 * Replaces, for these steps: DomainDecompBase::exchangeMolecules + LinkedCells::update (no migration, no re-sort) and the
 * HALO_COPIES message of NeighbourCommunicationScheme.cpp:115-136 by a position-only message. */
#define LS1HIP_REFRESH_DOUBLES 3
int ls1hip_verlet_build(ls1hip_ctx* ctx);
int ls1hip_halo_refresh(ls1hip_ctx* ctx);
/* Single-rank convenience: LinkedCells::update + DomainDecompBase::balanceAndExchange + updateMoleculeCaches in one call, list-aware.
 * While lists are alive and the displacement bound allows it (every drifting pass — the fused force pass as well as
 * ls1hip_kick_drift / ls1hip_kick_then_kick_drift — advances the bound on the device) only the halo positions are refreshed;
 * otherwise ls1hip_rebin + ls1hip_halo (+ ls1hip_verlet_build in list mode).  *rebuilt (may be NULL): 1 if it re-binned.
 * Follow with ls1hip_forces_list (list mode) or ls1hip_forces. */
int ls1hip_update(ls1hip_ctx* ctx, int* rebuilt);
int ls1hip_forces_list(ls1hip_ctx* ctx, int which, double dt, double* upot, double* virial);
/* List traversal of ALL cells that also does the step's post-force kick (Leapfrog::transition2to3 -> FullMolecule::upd_postF,
 * integrators/Leapfrog.cpp:66-150) in its epilogue: v += dt_half / m F with the kinetic sum of thermostat 0 (fetch it with
 * ls1hip_kinetic_sums), F is kept — the pass ls1hip_run takes on unfused steps (NVT, the last step), for drivers that call the
 * pieces themselves (the reference driver through LinkedCellsHip / LeapfrogHip: one pass over the molecules less per step).
 * Single-centre LJ list path, and the pair-stream list pass of ONE rigid multi-site component (v, D kicked, sum m v^2 and sum I w^2
 * of the step; same state as ls1hip_forces_list + ls1hip_kick bit for bit); read-only option "list_kick_available".  Otherwise
 * (several components, per-molecule virial) LS1HIP_EINVAL — use ls1hip_forces_list + ls1hip_kick. */
int ls1hip_forces_list_kick(ls1hip_ctx* ctx, double dt_half, double* upot, double* virial);
int ls1hip_verlet_poll(ls1hip_ctx* ctx, int* need_rebuild);

/* nsteps full time steps entirely on the device (single rank, all directions local), no host round trip
 * inside: the loop body of Simulation::simulate (Simulation.cpp:979-1167) for an NVE run without plugins.
 * out6 (may be NULL) = {upot, virial, summv2, sumIw2, N, rotDOF} of the LAST step. */
int ls1hip_run(ls1hip_ctx* ctx, double dt, unsigned long nsteps, double* out6);
/* The global values of EVERY step of the last ls1hip_run, one row {upot, virial, summv2, sumIw2, N, rotDOF} per step,
 * oldest first (the last 4096 steps are kept): what Leapfrog::transition2to3 hands to Domain::setLocalSummv2 / SumIw2
 * (integrators/Leapfrog.cpp:115-150) and VectorizedCellProcessor::endTraversal to setLocalUpot / Virial in every step,
 * i.e. the inputs of Domain::calculateGlobalValues (Domain.cpp:151-181, called per step at Simulation.cpp:1099-1103).
 * The rows are written by the reduction kernels on the device, no host round trip inside the run; in the fused mode
 * the kinetic sum comes out of the force pass's own epilogue.  Columns 2-5 are NaN for steps whose kinetic sums were not
 * computed (unfused NVE steps before the last).  rows may be NULL to query *nrows. */
int ls1hip_run_log(ls1hip_ctx* ctx, size_t cap_rows, double* rows, size_t* nrows);

/* ---- radial distribution functions ------------------------------------------------------------------------------
 * The reference's RDF plugin (io/RDF.{h,cpp}) and its RDFCellProcessor (particleContainer/adapter/RDFCellProcessor.cpp): a
 * second traversal of the linked cells that counts every molecule pair inside the cutoff r_c (the force cutoff, not r_c + skin)
 * into histograms over the centre distance, and with site_rdf the site-site distances of multi-site pairs as well.
 * Histogram layout (u64 words):
 *   mol[p][bin]   p runs over the component pairs (i, j >= i) in the order of RDF::collectRDF (RDF.cpp:235-241):
 *                 (0,0) (0,1) ... (0,C-1) (1,1) ... (C-1,C-1); bin = floor(sqrt(dd) / interval_length) (RDF.h:138-146);
 *   site          the blocks of the pairs with n_i + n_j > 2 sites (RDF.cpp:111-135), in the same order, each [m][n][bin] with m
 *                 a site of component i and n one of component j, sites ordered LJ centres, charges, dipoles, quadrupoles
 *                 (FullMolecule.h:171-185).  For i == j and m != n the raw counts carry the reference's double count
 *                 (RDF.h:152-170); its writer applies the factor 1/2 (RDF.cpp:558).
 * Every unordered pair is counted once in the sum over all ranks: the rank that owns the molecule with the smaller id counts it
 * (the reference's cell-index rule, RDFCellProcessor.cpp:104-109, serves the same end).  A molecule and its own periodic image
 * are not a pair: boxes are at least 2 r_c long per periodic dimension.  The grid has one cell per cutoff (cells_in_cutoff = 1).
 *
 * ls1hip_rdf_config: RDF::readXML + RDF::init (RDF.cpp:35-179) — bins, intervallength; site_rdf != 0 allocates the site blocks
 *   (the reference switches them on whenever a pair has more than two sites).  Needs components and domain; bins > 0,
 *   interval_length > 0, finite bins * interval_length.  bins = 0: sampling off, buffers freed.  Histograms start at zero. */
int ls1hip_rdf_config(ls1hip_ctx* ctx, int bins, double interval_length, int site_rdf);
/* Words of the two histograms of the current configuration (0, 0 when off). */
int ls1hip_rdf_layout(const ls1hip_ctx* ctx, size_t* mol_words, size_t* site_words);
/* One traversal (RDF::afterForces -> ParticleContainer::traverseCells(RDFCellProcessor), RDF.cpp:573-581): adds the pairs of the
 * CURRENT positions and orientations, wherever the engine keeps them, to the device histograms, the owned molecules per component
 * to the counters (RDF::accumulateNumberOfMolecules, RDF.cpp:195-199) and 1 to the sample counter (tickRDF).  Preconditions of
 * ls1hip_forces(ctx, 0, ...): molecules binned, halo valid — after rebin; halo[; forces], and between two builds of the neighbour
 * lists after ls1hip_update / ls1hip_halo_refresh (bins stale by at most skin / 2, grid sized by r_c + skin: no pair inside r_c
 * is missed).  Anything else is an error, never a partial count.  Timer "rdf". */
int ls1hip_rdf_sample(ls1hip_ctx* ctx);
/* LOCAL counts of this rank (the inputs of RDF::collectRDF, RDF.cpp:231-306, which sums them over the ranks); any pointer may be
 * NULL; n_per_component[ncomp]; *samples = traversals since the last reset. */
int ls1hip_rdf_read(ls1hip_ctx* ctx, uint64_t* mol, size_t cap_mol, uint64_t* site, size_t cap_site, uint64_t* n_per_component,
					uint64_t* samples);
/* RDF::reset (RDF.cpp:309-340): histograms, molecule counters and sample counter back to zero. */
int ls1hip_rdf_reset(ls1hip_ctx* ctx);
/* The angular RDF of the same plugin (<angularbins> > 1: io/RDF.h:93-109 observeARDFMolecule, adapter/RDFCellProcessor.cpp:36-41,
 * MoleculeInterface.h:167-190 orientationAngle, RDF.cpp:49-55, 88-91, 137-146, 253-272, 377-453).  Every pair the RDF pass observes
 * adds two counts, ardf[c_i][c_j][flat(b, a_ij)] and ardf[c_j][c_i][flat(b, a_ji)]: b the distance bin, a = floor((-cos phi + 1.) /
 * (2. / angularbins)) with cos phi between the CENTRAL molecule's orientation vector (from its quaternion as stored; (0, 0, 1) for
 * components without rotation) and the direction to the other one.  The first index is the component of the central molecule: the
 * nC x nC blocks are not symmetric.  flat = b angularbins + a in signed arithmetic, as the reference's flat index (RDF.h:97-100):
 * a = -1 (cos phi rounded above 1) or a = angularbins (cos phi <= -1) lands in the neighbouring distance row; only a flat index
 * outside [0, bins angularbins), where the reference writes outside its vector, is dropped.
 *
 * ls1hip_rdf_config_angular: after ls1hip_rdf_config (an error without it).  angularbins <= 1 switches the angular part off and
 *   frees it; nC^2 bins angularbins words must fit the 32-bit word index.  ls1hip_rdf_config drops the angular configuration (the
 *   bins changed).  With the angular part on, ls1hip_rdf_sample (and "rdf_every") fills these words in the same sample: one
 *   traversal for molecule histogram, counters and ARDF without site histograms, a second one behind the RDF pass with them; the
 *   sample counter ticks once; ls1hip_rdf_reset zeroes them too.  With it off nothing changes. */
int ls1hip_rdf_config_angular(ls1hip_ctx* ctx, int angularbins);
/* LOCAL counts of this rank (RDF::collectRDF sums them over the ranks, RDF.cpp:253-272), layout [c_central][c_other][b angularbins
 * + a]; *words = nC^2 bins angularbins; ardf may be NULL to query *words only.  An error while the angular part is off. */
int ls1hip_rdf_angular_read(ls1hip_ctx* ctx, uint64_t* ardf, size_t cap, size_t* words);
/* Option "rdf_every" (ls1hip_set_option, default 0 = never): ls1hip_run samples on every step s with s % rdf_every == 0, s counted
 * from 1 over all ls1hip_run calls of the context (simstep % _samplingFrequency of RDF::afterForces).  The pass runs on the
 * positions of that step's force evaluation, directly before the force pass, on the step's regenerated or refreshed halo; the
 * trajectory does not change. */

/* ---- orientation distribution functions ---------------------------------------------------------------------------
 * The reference's ODF plugin (io/ODF.{h,cpp}) and its ODFCellProcessor (particleContainer/adapter/ODFCellProcessor.cpp): a
 * traversal of the linked cells that histograms the mutual orientation of every pair of SINGLE-DIPOLE molecules (components with
 * exactly one dipole, ODFCellProcessor.cpp:25,34; dipole direction (0, 0, 1) in the body frame, ODF.cpp:42-45) whose centres are
 * closer than min(r_c, shellcutoff) (ODFCellProcessor.cpp:40, ODF.cpp:151).  Per pair, with d = r_j - r_i taken with the halo
 * image of j and e_k = (2(qx qz + qw qy), 2(qy qz - qw qx), 1 - 2(qx^2 + qy^2)) of the quaternion as stored (ODF.cpp:191-193):
 *   c1 = d^.e_i, c2 = -d^.e_j, cg = p^_i.p^_j with p_k = d^ x (e_k x d^) (ODF.cpp:197-229); each of the three is replaced by its
 *   nearest integer when |c| < 1e-4 or ||c| - 1| < 1e-4 (:234-242); gamma = acos(cg);
 *   i1: 1 - 2 i / P >= c1 > 1 - 2 (i + 1) / P, c1 == -1 -> P - 1; i2 likewise from c2; g = i + 1 with i pi / G <= gamma <
 *   (i + 1) pi / G, gamma == pi -> G (:253-290); a value that fits nowhere (NaN: e parallel to d) keeps index 0.
 * Layout (u64 words): four arrays of W = P P G + 1 words (ODF.cpp:51; word 0 is the reference's unused element) in the order
 * 11 12 21 22; a pair with component ids (a, b) in {0, 1} adds 1 to H[a][b][i1 P G + i2 G + g] and to H[b][a][i2 P G + i1 G + g]
 * (elementID, elementIDreversed, :305-329), so the sum does not depend on which molecule of a pair plays i.  Every unordered pair
 * is counted once in the sum over all ranks (the rank that owns the smaller id counts it), also across periodic faces.
 *
 * ls1hip_odf_config: ODF::readXML + ODF::init (ODF.cpp:6-79) — phi1increments, phi2increments, gammaincrements, shellcutoff.
 *   All increments 0: sampling off, buffers freed.  LS1HIP_EINVAL for phi1 != phi2 (the reference's reversed index, :306, is not
 *   the transposed one there and can leave its array), shell_cutoff <= 0 or > r_c, a single-dipole component with id >= 2 (the
 *   reference has the four arrays of the ids 0 and 1, :73-76), 4 W beyond the 32-bit word index.  Arrays start at zero. */
int ls1hip_odf_config(ls1hip_ctx* ctx, int phi1_increments, int phi2_increments, int gamma_increments, double shell_cutoff);
/* W of the current configuration (0 when off). */
int ls1hip_odf_layout(const ls1hip_ctx* ctx, size_t* words_per_array);
/* One traversal (ODF::afterForces -> traverseCells(ODFCellProcessor), ODF.cpp:81-85) of the CURRENT positions and orientations,
 * added to the device arrays; the sample counter goes up by 1.  State: that of ls1hip_rdf_sample (binned, halo valid, no split
 * pass in flight, cells_in_cutoff = 1).  Timer "odf". */
int ls1hip_odf_sample(ls1hip_ctx* ctx);
/* LOCAL counts of this rank (the inputs of ODF::collect, ODF.cpp:333-384), hist[4][W] in the order 11 12 21 22 (may be NULL);
 * *samples = traversals since the last reset. */
int ls1hip_odf_read(ls1hip_ctx* ctx, uint64_t* hist, size_t cap, uint64_t* samples);
/* ODF::reset (ODF.cpp:104-121): arrays and sample counter back to zero. */
int ls1hip_odf_reset(ls1hip_ctx* ctx);
/* Options "odf_every" (_recordingTimesteps; default 0 = never) and "odf_from" (_initStatistics, default 0): ls1hip_run samples on
 * every step s with s > odf_from && s % odf_every == 0 (ODF.cpp:82), s counted as for "rdf_every", at the place of the RDF pass;
 * an error without a configuration.  Read-only option "odf_lds_words": the 4 W up to which a workgroup keeps the arrays in LDS. */

/* ---- cavity detection ----------------------------------------------------------------------------------------------
 * The reference's CavityWriter plugin (io/CavityWriter.{h,cpp}) and its CavityEnsemble (ensemble/CavityEnsemble.{h,cpp}): a regular
 * lattice of Nx x Ny x Nz test nodes over the control volume [cb, ct) (default: the whole domain), node (tx, ty, tz) at
 * cb_d + (0.5009756 + t_d) (ct_d - cb_d) / N_d with the id tid = tx Ny Nz + ty Nz + tz + 1 (CavityEnsemble.cpp:158-171).  Per node
 * the number of container entries j with dd = dx dx + dy dy + dz dz < RR, RR = (double)((float)radius * (float)radius)
 * (setSystem, :49-51; countNeighbours, :280-311), where an entry counts iff it lies in the GLOBAL box, 0 <= r_j,d < L_d (the search
 * box clamped to [0, L], :289-292, and the region iterator's lo <= r < hi): NO periodic images — a node near a face sees fewer
 * neighbours — while halo copies received from a neighbouring rank count; ALL components count (the plugin's componentid list only
 * names output files); an entry whose id equals the node's tid is skipped (:298, an id clash of the reference, kept so that files
 * match).  A node is active (a cavity) iff count <= maxNeighbours (decideActivity, :254-259).
 *
 * ls1hip_cavity_config: CavityWriter::readXML (CavityWriter.cpp:40-90) + CavityEnsemble::setSystem / setControlVolume /
 *   setSubdomain / init (CavityEnsemble.cpp:49-112,135-160).  cv_min = cv_max = NULL: the whole domain.  This rank's nodes are
 *   t_d = round(N_d minredco_d - 0.0009756) ... round(N_d maxredco_d - 0.0009756) - 1 with the reduced coordinates of the context's
 *   subdomain held in float (:82-93,144-145), cut to [0, N_d).  LS1HIP_EINVAL for radius <= 0, radius > r_c (cells and halo shell
 *   guarantee r_c only), N_d <= 0, maxNeighbours <= 0 (CavityWriter.cpp:41-65), more than 2^32 - 1 nodes, an empty control volume or
 *   one that leaves the domain (:78-90). */
int ls1hip_cavity_config(ls1hip_ctx* ctx, int nx, int ny, int nz, int max_neighbours, float radius, const double cv_min[3],
						 const double cv_max[3]);
/* One CavityEnsemble::cavityStep (CavityEnsemble.cpp:313-330, called from CavityWriter::afterForces, CavityWriter.cpp:160-174) on the
 * CURRENT positions.  State: that of ls1hip_rdf_sample (binned, halo valid — between two list builds the refreshed one —, no split
 * pass in flight); any cells_in_cutoff.  Options "cavity_counts" (1: exact counts, no early exit; default 0: flags only) and
 * "cavity_chunk" (container entries per LDS staging chunk, 0 = read-only option "cavity_chunk_max").  Timer "cavity". */
int ls1hip_cavity_sample(ls1hip_ctx* ctx);
/* Result of the last sample: lo[3], n[3] = this rank's range of the lattice (minlu, maxlu - minlu + 1); flags[n0 n1 n2] (1: active)
 * and counts[n0 n1 n2] in ascending tid of that range — the order of CavityEnsemble::activeParticleContainer (:271-278) that
 * CavityWriter::endStep writes rank by rank (CavityWriter.cpp:211-235); counts: LS1HIP_EINVAL unless that sample ran in count
 * mode; *n_active = this rank's active.size(), the input of communicateNumCavities (:221-229).  Every pointer may be NULL. */
int ls1hip_cavity_read(ls1hip_ctx* ctx, uint32_t lo[3], uint32_t n[3], uint8_t* flags, uint32_t* counts, size_t cap, uint64_t* n_active);
/* n_active of the samples since the configuration, oldest first (the last 4096 at most); *samples = how many. */
int ls1hip_cavity_series(ls1hip_ctx* ctx, size_t cap, uint64_t* n_active, size_t* samples);
/* Options "cavity_every" (_writeFrequency; default 0 = never) and "cavity_from" (Simulation::getInitStatistics): ls1hip_run samples
 * on every step s with s >= cavity_from && s % cavity_every == 0 (CavityWriter.cpp:165), s counted as for "rdf_every", on the
 * positions of that step's force evaluation — what afterForces sees; the pass runs directly before the force pass because a fused
 * pass leaves the next step's positions behind.  An error without a configuration.  The trajectory does not change. */

/* ---- spatial profiles ----------------------------------------------------------------------------------------------
 * The reference's SpatialProfile plugin (plugins/SpatialProfile.{h,cpp}) with the profiles of plugins/profiles/: per bin of a
 * Cartesian or cylindrical sampling grid over the GLOBAL box the number of molecules and, on request, sums of |v|, v, 3 + rotDOF,
 * m v^2 + I w^2 and the per-molecule virial.  The accumulators are global (one entry per bin of the whole box) and live on the
 * device; every rank counts its OWNED molecules only, never halo copies, so the sum of the tables over the ranks is what the
 * reference's collCommAllreduceSum delivers (SpatialProfile.cpp:286-310).
 * Bin index (SpatialProfile::init, getCartesianUID, getCylUID; SpatialProfile.cpp:146-222, 339-410), operation for operation:
 *   Cartesian  inv[d] = units[d] / global_len[d];  uID = floor(x inv0) ny nz + floor(y inv1) nz + floor(z inv2);
 *   cylinder   centre (Lx/2, 0, Lz/2), R2max = 0.24 min(Lx, Lz)^2, inv = (nR / R2max, nH / Ly, nPhi / 2 pi),
 *              phi = atan2(zc, xc) (+ 2 pi when negative), uID = hUn nR nPhi + rUn nPhi + phiUn; molecules with rUn >= nR are
 *              skipped.
 * Coordinates are the global ones wrapped into [0, L): between two builds of the neighbour lists a molecule may sit up to
 * skin / 2 outside the box and is binned where ls1hip_download_state reports it.  DEVIATION: an index that rounds to n at the
 * upper face of the box is clamped to n - 1 (the reference writes such a molecule into a map entry no writer reads).
 * Summation order: the u64 counts are exact; the f64 sums are accumulated with atomic adds whose arrival order is not fixed, so
 * they may differ in the last bits from run to run. */
#define LS1HIP_PROF_CARTESIAN 0
#define LS1HIP_PROF_CYLINDER  1
/* quantities (bit mask); the molecule count N is always sampled (DensityProfile.h:19-21) */
#define LS1HIP_PROF_VELOCITY    1   /* sum |v|              VelocityAbsProfile.h:22-31                    */
#define LS1HIP_PROF_VELOCITY3D  2   /* sum v[3]             Velocity3dProfile.h:24-28                     */
#define LS1HIP_PROF_TEMPERATURE 4   /* sum (3 + rotDOF) as u64, sum (m v^2 + I w^2)   DOFProfile.h:18-20, KineticProfile.h:17-22 */
#define LS1HIP_PROF_VIRIAL      8   /* sum Vi[3]            VirialProfile.h:27-31                         */
/* SpatialProfile::readXML + init (SpatialProfile.cpp:22-222): units = (x, y, z) bins in Cartesian mode, (r, h, phi) in cylinder
 * mode; component = -1 samples every component, otherwise the 0-based component id (the reference's XML value is 1-based and
 * compared as componentid() == _profiledComp - 1, SpatialProfile.cpp:244).  units = {0, 0, 0}: sampling off, buffers freed.
 * Needs components and domain.  LS1HIP_EINVAL: a zero unit among non-zero ones, bins x words per bin above the 32-bit index, an
 * unknown mode or quantity bit, a component id outside the component set.  Tables start at zero. */
int ls1hip_profile_config(ls1hip_ctx* ctx, int mode, const uint32_t units[3], unsigned quantities, int component);
/* Bins and quantity mask of the current configuration (0, 0 when off): _uIDs of SpatialProfile.cpp:189-190. */
int ls1hip_profile_layout(const ls1hip_ctx* ctx, size_t* bins, unsigned* quantities);
/* The molecule loop of SpatialProfile::endStep (SpatialProfile.cpp:238-283): one pass over the owned molecules, on the CURRENT
 * positions and velocities wherever the engine keeps them; adds 1 to the sample counter (_accumulatedDatasets).  The caller is
 * responsible for full-step velocities (the reference samples after the post-force kick and after the thermostat,
 * Simulation.cpp:1099-1131, 1223).  Refused instead of sampling a wrong state: after a fused force + integration pass
 * (velocities half a step ahead, positions parked), while a split pass is in flight, and LS1HIP_PROF_VIRIAL without option
 * compute_vi = 1 and valid forces.  m v^2 and I w^2 are the terms of ls1hip_kinetic_sums_by_component; rotDOF comes from the
 * component table (ls1hip_set_rot_dof).  Timer "profile". */
int ls1hip_profile_sample(ls1hip_ctx* ctx);
/* LOCAL tables of this rank (the operands of collectAppend, SpatialProfile.cpp:293-297); any pointer may be NULL, one that is
 * not needs its quantity configured; n, dof, ekin, vabs: [bins]; v3, vi3: [bins][3]; cap_bins: entries the buffers hold;
 * *samples = ls1hip_profile_sample passes since the last reset. */
int ls1hip_profile_read(ls1hip_ctx* ctx, size_t cap_bins, uint64_t* n, uint64_t* dof, double* ekin, double* vabs, double* v3,
						double* vi3, uint64_t* samples);
/* ProfileBase::reset of every bin and _accumulatedDatasets = 0 (SpatialProfile.cpp:320-326). */
int ls1hip_profile_reset(ls1hip_ctx* ctx);
/* Options "profile_every" (default 0 = never) and "profile_from" (default 0): ls1hip_run samples on every step s with
 * s >= profile_from && s % profile_every == 0, s counted as for "rdf_every" (simstep >= _initStatistics && simstep %
 * _profileRecordingTimesteps == 0, SpatialProfile.cpp:238).  The sample is taken AFTER that step's post-force kick; with the
 * device thermostat it bins beta_trans v and beta_rot D with the factors the kick's reduction left on the device — the scaled
 * velocities the reference's endStep sees — without touching the state.  A sampling step takes the loop's unfused route (as the
 * last step of a call does); per-step loops keep their trajectory bit for bit, list loops may move a rebuild. */

/* ---- planar long-range correction ------------------------------------------------------------------------------------
 * The reference's correction for vapour-liquid interfaces and films, longRange/Planar.{h,cpp} with _smooth = false: a density
 * profile along y per LJ site and per dipolar component (a component with dipoles or charges), from it per-slab tables of force,
 * energy and normal / tangential virial (centerCenter, centerSite, siteSite, dipoleDipole), applied to every site in every step.
 * Rows: the LJ sites in component order (numLJSum2), then one row per dipolar component (numDipoleSum2).  The device keeps u64
 * COUNTS per (row, slab) of the OWNED molecules — exact, reproducible, additive over ranks — and forms rho = count slabs / V
 * when the tables are built; the slab sum is a gather in a fixed order, so equal counts give bit-equal tables.  Kept from the
 * reference: pi = 3.1416, (int) truncation of y / delta with its one-slab wrap, the self terms as Planar.cpp:495-497, 556-560,
 * 618-622, 805-809 write them, cutoff_slabs as a double, slabs / 2 as integer division, muSquare indexed by component id.
 * DEVIATIONS: a centre whose y / delta rounds to `slabs` is counted in the last slab; LS1HIP_EINVAL for component sets in which a
 * component without dipole / charge precedes one with (the reference reads outside muSquare there); the right-half self term of
 * centerCenter is dropped where its row index (Planar.cpp:556) lies beyond the LJ rows (the reference writes outside its arrays).
 * Not served: _smooth = true, the DistControl-tracked region, a fused-epilogue form. */
/* Planar::readXML + init (Planar.cpp:40-218): slabs (0: off, buffers freed), frequency (density and tables are recomputed on
 * every frequency-th call), the region [left, right] in y in which the FORCE is applied (u and the virial always are),
 * temperature = the target temperature dipoleDipole uses (only read for dipolar components).  The cutoff is the LJ cutoff of the
 * context.  Needs components and domain; restarts the call counter. */
int ls1hip_planar_config(ls1hip_ctx* ctx, int slabs, int frequency, double region_left, double region_right, double temperature);
/* One Planar::calculateLongRange() (Planar.cpp:220-476) of a single-rank domain, called where Simulation.cpp:841, 1048-1049 call it:
 * after a force pass, before the forces are used.  Counts calls as the reference counts simsteps: density + tables when
 * counter % frequency == 0 (so with the first call), then the tables are applied: F_y of every LJ site (inside the region), its
 * torque in M, u and 2 vT + vN into the two results (Domain::setUpotCorr / setVirialCorr), (vT, vN, vT) into Vi with option
 * compute_vi.  Needs valid forces; refused after a fused force + integration pass.  Timers "planar_density", "planar_tables",
 * "planar_apply". */
int ls1hip_long_range_planar(ls1hip_ctx* ctx, double* upot_corr, double* virial_corr);
/* The same piecewise, for multi-rank hosts: _density ADDS the counts of this rank's owned molecules to whatever the device holds (the
 * loop Planar.cpp:281-308) — the host must write ZEROS (_counts_write) before every sampling, or the previous global sum is counted
 * again —, _counts_read / _counts_write move the [rows][slabs] u64 counts for the host's all-reduce (which replaces
 * collCommAllreduceSum :320-336) and put the global sum on the device, _tables builds all tables from the counts
 * now on the device — every rank the whole table, so the reference's second all-reduce (:374-400) disappears —, _apply is the
 * molecule loop :404-460 and returns this rank's share of Upot_c / Virial_c (the operands of :463-469). */
int ls1hip_planar_density(ls1hip_ctx* ctx);
int ls1hip_planar_counts_read(ls1hip_ctx* ctx, size_t cap, uint64_t* counts);
int ls1hip_planar_counts_write(ls1hip_ctx* ctx, size_t n, const uint64_t* counts);
int ls1hip_planar_tables(ls1hip_ctx* ctx);
int ls1hip_planar_apply(ls1hip_ctx* ctx, double* upot_corr, double* virial_corr);
/* layout = {slabs, LJ rows, dipole rows} (zeros when off; may be NULL); rho, u, vN, vT, f: [LJ rows + dipole rows][slabs], the LJ
 * rows first (rho_l, uLJ, vNLJ, vTLJ, fLJ | rhoDipoleL, uDipole, vNDipole, vTDipole, fDipole); any pointer may be NULL. */
int ls1hip_planar_read(ls1hip_ctx* ctx, int layout[3], size_t cap, double* rho, double* u, double* vN, double* vT, double* f);
/* Inside ls1hip_run a configured correction is called after every force pass; fused passes and the list pass's own kick are off
 * (every step goes the unfused route of NVT steps).  {Upot_c, Virial_c} of every step go to a device ring beside the step log;
 * rows2 [nrows][2], oldest first, as ls1hip_run_log. */
int ls1hip_planar_log(ls1hip_ctx* ctx, size_t cap_rows, double* rows2, size_t* nrows);

/* ---- external walls: LJ 9-3 / 10-4-3 wall potential, mirrors -----------------------------------------------------------------
 * What closes the reference's film, adsorption and evaporation set-ups in y: plugins/WallPotential.{h,cpp} (an integrated Lennard-Jones
 * wall felt by every LJ site, hook siteWiseForces) and plugins/Mirror.{h,cpp} (a reflecting plane or a harmonic restoring force, hook
 * afterForces).  Both act between the force pass and the kick, so they are ONE device pass over the owned molecules (kernels_wall.hip)
 * that reads y alone of every molecule out of reach and leaves its F, M and v bit for bit.  Positions are global coordinates, so every
 * rank of a decomposed run applies the pass to its own molecules.  The wall's energy, Sum over sites of (u - u_shift) per component, has
 * an output of its own: the reference keeps it in Domain::setLocalUpotCompSpecific only, it is part of neither U_pot nor the virial.
 * DEVIATION: the 10-4-3 energy and its shift are computed with 2./5.; the reference's integer 2 / 5 is 0 (WallPotential.cpp:184, 318)
 * and nothing it writes shows that energy.  Forces are the reference's expressions as written.
 * Not served: the deprecated mirror types 3 and 4, MT_MELAND_2004 (5) and MT_RAMPING (6) — they delete molecules and draw random numbers —,
 * mirror positions tracked by DistControl (position/refID != 0), more than 4 mirrors, the wall's halo molecules in the energy sum (the
 * reference iterates ALL_CELLS; the device sums owned molecules). */
/* WallPotential::readXML + initializeLJ93 / initializeLJ1043 (WallPotential.cpp:10-187).  potential: 0 off, 93, 104 (anything else is
 * refused; the reference falls back to 9-3); density, sigma, epsilon: the wall's; yoff, ycut, width, delta as in the XML (delta is read
 * by the 10-4-3 form only).  ncomp must be the component count; consider[c] != 0: component c feels the wall (NULL: every component,
 * the XML without <component> entries); xi, eta: [ncomp] (read for the considered components).  eps_wi, sig_wi and the energy shift come
 * from LJ centre 0 of the component: a considered component without an LJ centre is LS1HIP_EINVAL (the reference reads ljcenter(0) of
 * nothing).  Needs components and domain.  The mirrors are kept. */
int ls1hip_wall_config(ls1hip_ctx* ctx, int potential, double density, double sigma, double epsilon, double yoff, double ycut, double width,
                       double delta, int ncomp, const int* consider, const double* xi, const double* eta);
/* Mirror::readXML (Mirror.cpp:53-187) of one of 4 mirrors.  slot 0..3; type 0 off, 1 MT_REFLECT, 2 MT_FORCE_CONSTANT (3..6:
 * LS1HIP_EINVAL with a message, see above); direction 0 left |-o (the mirror owns y < coord and sends molecules to the right), 1 right
 * o-| (y >= coord); coord = position/coord with refID 0; cid 0 = every component, else the 1-based component id of the XML;
 * force_constant: read by type 2. */
int ls1hip_mirror_config(ls1hip_ctx* ctx, int slot, int type, int direction, double coord, int cid, double force_constant);
/* The pass on the current F and v: calcTSLJ_9_3 / calcTSLJ_10_4 (WallPotential.cpp:193-341), then Mirror::VelocityChange of every
 * mirror in slot order (Mirror.cpp:421-477; membership by the half-open test of MoleculeInterface::inBox on the wrapped centre).
 * Hosts call it after a force pass, as they call ls1hip_long_range_planar; it needs valid forces and is refused after a fused force +
 * integration pass.  upot_comp: [ncomp] wall energy per component of this rank's molecules, or NULL.
 * The reference's driver does NOT apply the wall to the initial forces (siteWiseForces returns at simstep 0, prepare_start does not call
 * it) but it DOES call the mirrors there (Simulation.cpp:880-886): a host that reproduces it calls this once on the initial state
 * with the mirrors configured and the wall not (yet).  Timer "wall". */
int ls1hip_wall_apply(ls1hip_ctx* ctx, double* upot_comp);
/* Inside ls1hip_run a configured wall or mirror is applied after every force pass (after the planar correction: the reference runs
 * wall, correction, mirror — Simulation.cpp:1041-1079 — which differs in the rounding order of the additions to F only); fused passes
 * and the list pass's own kick are off, as with the planar correction.  The per-component energies of every step go to a device ring
 * beside the step log; rows [nrows][ncomp], oldest first, as ls1hip_run_log; nrows = 0 if the last ls1hip_run had neither a wall nor a mirror. */
int ls1hip_wall_log(ls1hip_ctx* ctx, size_t cap_rows, double* rows, size_t* nrows);

/* ---- test-particle insertions, Widom sampling -----------------------------------------------------------------
 * The energy a molecule WOULD have at a point, without adding it: what ChemicalPotential::grandcanonicalStep
 * (ensemble/ChemicalPotential.cpp:451-591) asks LinkedCells::getEnergy for, once per ghost molecule
 * (particleContainer/LinkedCells.cpp:998-1052 -> LegacyCellProcessor::processSingleMolecule, adapter/LegacyCellProcessor.cpp:34-54):
 * dU = U6 / 6 + U_xpoles + U_RF of FluidPot (molecules/potforce.h:506-650, ParticlePairs2PotForceAdapter.h:170-176) over the
 * molecules and halo copies whose centre lies inside r_c, with the parameter products, shift6, LJ cutoff on the centre distance
 * and reaction-field term of the force kernels.  No long-range correction is added (the host may add 2 U_corr / N).
 * DEVIATION: a partner whose centre coincides with the test's (dd == 0) is skipped, the mask of every force path here
 * (VectorizedCellProcessor); the legacy processor would evaluate it.
 * State: that of ls1hip_rdf_sample — molecules binned (or neighbour lists alive on a single-rank domain: the stale binning of
 * the last build is complete, a partner inside r_c now was inside r_c + skin / 2 of the point then), halo valid, no split force
 * pass in flight; the current positions are used wherever the engine keeps them.  cells_in_cutoff 1 and 2.  Nothing is written
 * to the state.  Timer "insert". */
/* n tests from HOST arrays: cid[n], r[n][3] inside this rank's [box_min, box_max), q[n][4] (normalised where the rotation is
 * formed; NULL only if no test's component rotates), exclude_id[n] or NULL: id of a molecule the test does not see, with its
 * periodic images (LegacyCellProcessor.cpp:44) — the energy of an EXISTING molecule is the call at its position with its id.
 * dU[n]; exactly 0 where no partner is in range.  One wave per test, no atomics: the same state gives the same bits.
 * LS1HIP_EINVAL names the first test with a component id out of range, a position outside the box or a missing q.  n = 0: OK. */
int ls1hip_insertion_energies(ls1hip_ctx* ctx, size_t n, const int32_t* cid, const double* r, const double* q,
							  const uint64_t* exclude_id, double* dU);
/* Widom's method (the accumulation Domain::submitDU was meant for, Domain.cpp:810-829, its body commented out in the reference):
 * every sample inserts `instances` ghost molecules of `component` at positions uniform in [cv_min, cv_max) (NULL, NULL: this
 * rank's box; otherwise inside it) and adds w = exp(-dU / temperature) to slab floor(y / L_y * slabs) of the GLOBAL box.
 * Test k of sample s is a pure function of (seed, s, k): counter-based, independent of the launch shape.  DEVIATION: a component
 * with rotational degrees of freedom gets a uniformly distributed orientation; the reference inserts its reservoir molecule's
 * fixed one (ChemicalPotential.cpp:393-402), which does not sample the ideal-gas orientation distribution.
 * instances = 0: off, buffers freed.  Sums and sample counter start at zero. */
int ls1hip_widom_config(ls1hip_ctx* ctx, int component, uint32_t instances, double temperature, uint64_t seed, int slabs,
						const double cv_min[3], const double cv_max[3]);
/* One sample on the current state (sample index = samples since the last reset). */
int ls1hip_widom_sample(ls1hip_ctx* ctx);
/* LOCAL sums of this rank, additive over ranks and samples: sum_w[slabs] (f64, accumulated with atomics: the last bits depend
 * on the order), n[slabs] tests per slab; any pointer may be NULL. */
int ls1hip_widom_read(ls1hip_ctx* ctx, size_t cap_slabs, double* sum_w, uint64_t* n, uint64_t* samples);
/* The tests of the LAST sample: r[n][3], q[n][4], dU[n]; *n = their number (0 before the first sample); any pointer may be NULL. */
int ls1hip_widom_last(ls1hip_ctx* ctx, size_t cap, double* r, double* q, double* dU, size_t* n);
/* Sums, counts and the sample counter (hence the sample index) back to zero. */
int ls1hip_widom_reset(ls1hip_ctx* ctx);
/* Option "widom_every" (default 0 = never): ls1hip_run samples on every step s with s % widom_every == 0, at the place and with
 * the step counting of "rdf_every"; an error without a configuration.  The pass only reads: the trajectory keeps its bits. */

/* ---- region-wise temperature control (slab thermostat) -----------------------------------------------------------------------
 * Replaces: thermostats/TemperatureControl.{h,cpp}, method VelocityScaling, as Simulation.cpp:1137-1140 calls it (after the
 * post-force kick and Domain::calculateGlobalValues).  Every control region is a cuboid cut into `numslabs` slabs along y; each
 * slab has its own kinetic sums {n, rotDOF, ekinTrans = sum m v_d^2 over the masked directions, ekinRot = sum I w^2}, its own
 *   betaTrans = pow(ndir n T / ekinTrans, exponent) (1 when n < 1), betaRot = pow(rotDOF T / ekinRot, exponent) (1 when rotDOF < 1)
 * (TemperatureControl.cpp:283-301) and scales the masked velocity components by 2 - 1 / betaTrans and D by 2 - 1 / betaRot
 * (:392-409).  A molecule takes part when it is STRICTLY inside the region (:316-320, 371-375) with the component filter passed
 * (:311-313); its slab is (unsigned) floor((y - lc_y) / width), ignored beyond numslabs - 1 (:329-333).  Positions are those of
 * the current force evaluation, wrapped into the global box (in list mode molecules sit up to skin / 2 outside it); only owned
 * molecules take part.  A step is a control step when simstep % frequency == 0 (:639, 645, 651); measurement and new betas happen
 * only when also start <= simstep < stop (:719) — on a control step outside that window the scaling uses the betas of the LAST
 * measurement (1 with count 0 before the first).  All regions measure before any region scales; regions scale in their order, a
 * molecule inside two regions is scaled twice.
 * Limits: at most 8 regions.  The measure sweep keeps the slab sums of all regions in LDS per workgroup up to 1024 slabs in total
 * and adds to global memory directly above that; the apply passes stage the factors in LDS up to 256 slabs in total.  Counts are
 * exact; the f64 slab sums are accumulated with atomics and may differ in the last bits from run to run.  Not served: the method
 * Andersen, the addedEkin files, DistControl-tracked corners (refcoordsID).
 * State rules: those of ls1hip_kick — velocities full-step (call after the post-force kick), positions valid, no split or fused
 * pass in flight; nothing but v and D is written.  Excludes ls1hip_set_thermostat(enabled).  Timers "tempcontrol_measure",
 * "tempcontrol_betas", "tempcontrol_apply". */
#define LS1HIP_TC_X 1
#define LS1HIP_TC_Y 2
#define LS1HIP_TC_Z 4
/* control/start, frequency, stop (TemperatureControl.cpp:579-586).  frequency = 0 removes the thermostat and its regions. */
int ls1hip_tempcontrol_config(ls1hip_ctx* ctx, unsigned long start, unsigned long frequency, unsigned long stop);
/* Appends a region (ControlRegionT::readXML + VelocityScalingInit, :90-236; AddRegion :636) and returns its 1-based id (> 0), or
 * an error code (< 0).  component: 0 every component, else the 1-based id; direction_mask: LS1HIP_TC_X | _Y | _Z (the
 * reference's x, y, z, xy, xz, yz, xyz).  Appending a region puts EVERY region back to the state before its first measurement. */
int ls1hip_tempcontrol_region(ls1hip_ctx* ctx, const double lc[3], const double uc[3], double target_T, int component, unsigned numslabs,
							  double exponent, unsigned direction_mask);
/* _dTargetTemperature of one region; the temperature ramp (:266-277) stays on the host and calls this. */
int ls1hip_tempcontrol_target(ls1hip_ctx* ctx, int region, double target_T);
/* TemperatureControl::DoLoopsOverMolecules (:685-707) for step `simstep`: nothing on a step that is no control step. */
int ls1hip_temperature_control(ls1hip_ctx* ctx, unsigned long simstep);
/* The pieces, for hosts that reduce over ranks (the caller applies the window rule):
 *   _measure      the molecule loop of VelocityScalingPreparation (:725-728): LOCAL sums ADDED to the table
 *   _sums_read / _sums_write   the buffer of the all-reduce of CalcGlobalValues (:240-264): per slab of every region, regions in
 *                 their order, 32 bytes {u64 n, u64 rotDOF, f64 ekinRot, f64 ekinTrans}
 *   _betas        CalcGlobalValues after the all-reduce (:279-305): betas, factors, the sum-over-slabs accumulators, the sampled
 *                 configuration counter; keeps the sums as those of the last measurement and zeroes the table
 *   _apply        the molecule loop of DoLoopsOverMolecules (:700-703) with the factors of the last _betas
 *   _apply_kick_drift   _apply followed by ls1hip_kick_drift(dt) in one pass: the same bits */
int ls1hip_tempcontrol_measure(ls1hip_ctx* ctx);
int ls1hip_tempcontrol_sums_read(ls1hip_ctx* ctx, size_t cap_slabs, void* sums);
int ls1hip_tempcontrol_sums_write(ls1hip_ctx* ctx, size_t nslabs, const void* sums);
int ls1hip_tempcontrol_betas(ls1hip_ctx* ctx);
int ls1hip_tempcontrol_apply(ls1hip_ctx* ctx);
int ls1hip_tempcontrol_apply_kick_drift(ls1hip_ctx* ctx, double dt);
/* One region: the slab sums of the last measurement and its betas ([numslabs] each), beta_sums2 = {_dBetaTransSumGlobal,
 * _dBetaRotSumGlobal} (sums over slabs AND measurements) with their configuration count — what WriteBetaLogfile reads (:455-488);
 * reset != 0 puts the accumulators and the count back to zero as it does.  Any pointer may be NULL. */
int ls1hip_tempcontrol_read(ls1hip_ctx* ctx, int region, size_t cap_slabs, uint64_t* n, uint64_t* rot_dof, double* ekin_trans, double* ekin_rot,
							double* beta_trans, double* beta_rot, double* beta_sums2, uint64_t* configs, int reset);
/* regions configured, their slab counts (slabs8[8]), and the two LDS limits above (slabs of all regions together). */
int ls1hip_tempcontrol_layout(const ls1hip_ctx* ctx, int* regions, uint32_t* slabs8, size_t* lds_slabs, size_t* apply_lds_slabs);
/* ls1hip_run with temperature control configured: every step goes the unfused route (as NVT steps do); simstep is the run's step
 * counter, as for the profiles.  On a control step the measure sweep and the beta kernel follow the post-force kick; the scaling
 * is folded into the next step's kick + drift, and is a standalone pass after the last step and before a profile sampling pass
 * (SpatialProfile::endStep sees the scaled velocities).  The step log keeps the UNSCALED kinetic sums (calculateGlobalValues runs
 * before the control).  Works together with the planar correction.  Without a configuration ls1hip_run is what it was. */

/* ---- multi-GPU plumbing: packed buffers a host transport (RCCL via torch.distributed, MPI, ...) moves ---------
 * Wire formats (little endian, FP64): leaving molecule = 15 doubles {id(as bits), cid(as bits), r3, v3, q4, D3}
 * (the reference's 116-byte record, parallel/CommunicationBuffer.cpp:131-145, padded to 120); halo molecule =
 * 9 doubles {id, cid, r3, q4} (reference 68-byte record, CommunicationBuffer.cpp:167-176, padded to 72).
 * Positions are already shifted into the receiver's frame.
 * Replaces: CommunicationPartner::initSend / unpack (parallel/CommunicationPartner.cpp:139-227,266-389). */
#define LS1HIP_LEAVING_DOUBLES 15
#define LS1HIP_HALO_DOUBLES 9
/* kind: 0 = leaving molecules (valid after ls1hip_rebin), 1 = halo copies (valid after ls1hip_halo), 2 = position refresh of
 * the halo copies of the last list build (valid after ls1hip_halo_refresh; the counts are those of that build).
 * counts[27]: molecules packed per direction (0 for local / open directions). */
int ls1hip_export_counts(ls1hip_ctx* ctx, int kind, uint64_t counts[27]);
/* Copy the packed records of direction `dir` into the DEVICE buffer dev_buf (capacity in records). */
int ls1hip_export_pack(ls1hip_ctx* ctx, int kind, int dir, void* dev_buf, size_t cap);
/* The same for a list of directions, records back to back in the order given: one message per PEER (all directions
 * that point at the same neighbour rank), one stream synchronisation per message instead of one per direction.
 * Replaces the per-neighbour send loop of DirectNeighbourCommunicationScheme::initExchangeMoleculesMPI
 * (parallel/NeighbourCommunicationScheme.cpp:115-136). */
int ls1hip_export_pack_dirs(ls1hip_ctx* ctx, int kind, const int* dirs, int ndirs, void* dev_buf, size_t cap);
/* Append `n` received records from DEVICE buffer dev_buf: kind 0 -> owned molecules (then call ls1hip_rebin
 * again is NOT needed: they are binned on arrival), kind 1 -> halo copies.  The call is asynchronous: dev_buf is read
 * on the engine's stream and must stay valid until ls1hip_import_done(kind) returns.  Call ls1hip_import_done(kind)
 * after the last import of a kind. */
int ls1hip_import(ls1hip_ctx* ctx, int kind, const void* dev_buf, size_t n);
int ls1hip_import_done(ls1hip_ctx* ctx, int kind);

/* ---- seam A: CellProcessor-level drop-in (no container replacement) -------------------------------------------
 * One call = one complete traversal over the cells the reference's LinkedCells holds, given as a flat cell-major
 * molecule list.  Replaces the body of VectorizedCellProcessor::processCell / processCellPair / endTraversal
 * (adapter/VectorizedCellProcessor.cpp:124-157,2734-2821) when the adapter batches at endTraversal
 * (seam A).  cell_dims[3]: the reference's _cellsPerDimension incl. halo; cell_start[ncells+1]:
 * first molecule of each cell in the flat arrays; r/q/cid: molecule data incl. halo molecules;
 * outputs F/M/Vi [n][3] (halo entries are written as 0) and upot/virial with the reference's macroscopic rule. */
int ls1hip_soa_forces(ls1hip_ctx* ctx, const int cell_dims[3], const uint32_t* cell_start, size_t n, const double* r,
					  const double* q, const int32_t* cid, double* F, double* M, double* Vi, double* upot,
					  double* virial);

/* ---- measurement ---------------------------------------------------------------------------------------------- */

/* Device time (ms, HIP events on the context's compute stream) and launch count accumulated per kernel class
 * since the last reset: names[] in {"force","integrate","rebin","halo","build" (neighbour-list construction),
 * "rdf" (RDF sampling pass), "odf" (ODF sampling pass), "cavity" (cavity pass),
 * "profile" (profile sampling pass), "insert" (insertion-energy pass)}. */
int ls1hip_timing(ls1hip_ctx* ctx, const char* name, double* total_ms, uint64_t* launches);
int ls1hip_timing_reset(ls1hip_ctx* ctx);
/* Per-launch HIP-event timing: 0 = off, 1 = every phase, 2 = force passes only (each timed scope puts two event markers
 * into the stream, ~10 us of device idle per scope: a measured run that needs the force-kernel duration only uses 2). */
int ls1hip_timing_enable(ls1hip_ctx* ctx, int on);
/* Pair statistics of the last force call: distance checks and in-range molecule pairs (as FlopCounter counts
 * them, adapter/FlopCounter.cpp:20-76); requires option "count_pairs"=1. */
int ls1hip_pair_stats(ls1hip_ctx* ctx, uint64_t* dist_checks, uint64_t* pairs_in_range);

#ifdef __cplusplus
}
#endif
#endif /* LS1HIP_H_ */
