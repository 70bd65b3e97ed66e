"""Host-side mirror of the reference's plug-in interfaces for the linked-cell pair-force path.

Same class / method names, argument meaning and call order as the reference so that tests read like the
reference's own (``/root/reference/src/particleContainer/tests/LinkedCellsTest.cpp:511-600``):

    container.update(); decomp.balanceAndExchange(0., False, container, domain)
    container.updateMoleculeCaches(); container.traverseCells(cellProcessor)

Everything here is plumbing over the C ABI (``engine.DeviceEngine``); the compute is HIP.

Mirrored interfaces (reference file:line):
  ParticleContainer / LinkedCells   particleContainer/ParticleContainer.h:69-278, LinkedCells.cpp:243-356,564-628
  CellProcessor / VectorizedCellProcessor   adapter/CellProcessor.h:29-94, VectorizedCellProcessor.cpp:111-157
  Integrator / Leapfrog             integrators/Integrator.h:32-83, Leapfrog.cpp:35-150
  DomainDecompBase                  parallel/DomainDecompBase.cpp:51-86 (sequential periodic boundary)
  Domain (local macroscopic values) Domain.h:129-150, Domain.cpp:126-134
"""
from __future__ import annotations

import numpy as np

from .engine import DeviceEngine
from .inp import ComponentSet


class Domain:
    """The slice of the reference's Domain this path talks to (setLocal*/getLocal*)."""

    def __init__(self, global_length):
        self._globalLength = np.asarray(global_length, dtype=np.float64).copy()
        self._localUpot = 0.0
        self._localVirial = 0.0
        self._local2KETrans = {0: 0.0}
        self._local2KERot = {0: 0.0}
        self._localN = {0: 0}
        self._localRotDOF = {0: 0}

    def getGlobalLength(self, d):
        return float(self._globalLength[d])

    def getGlobalVolume(self):
        return float(self._globalLength[0] * self._globalLength[1] * self._globalLength[2])

    def setLocalUpot(self, u):
        self._localUpot = float(u)

    def getLocalUpot(self):
        return self._localUpot

    def setLocalVirial(self, v):
        self._localVirial = float(v)

    def getLocalVirial(self):
        return self._localVirial

    def setLocalSummv2(self, summv2, thermostat=0):
        self._local2KETrans[thermostat] = float(summv2)

    def setLocalSumIw2(self, sumIw2, thermostat=0):
        self._local2KERot[thermostat] = float(sumIw2)

    def setLocalNrotDOF(self, thermostat, N, rotDOF):
        self._localN[thermostat] = int(N)
        self._localRotDOF[thermostat] = int(rotDOF)

    def getLocalSummv2(self, thermostat=0):
        return self._local2KETrans[thermostat]

    # --- Domain::calculateGlobalValues, thermostat 0, single rank (Domain.cpp:151-240)
    def setGlobalTemperature(self, T):
        self._universalTargetTemperature = float(T)

    def calculateGlobalValues(self, domainDecomp=None, particleContainer=None, collectThermostatVelocities=True,
                              Tfactor=1.0):
        self._globalUpot = self._localUpot
        self._globalVirial = self._localVirial
        N, rotDOF = self._localN[0], self._localRotDOF[0]
        summv2 = self._local2KETrans[0]
        sumIw2 = self._local2KERot[0] if rotDOF > 0 else 0.0
        self._globalTemperature = (summv2 + sumIw2) / (3 * N + rotDOF) if N > 0 else 0.0
        Ti = Tfactor * getattr(self, "_universalTargetTemperature", 0.0)
        if Ti > 0.0 and N > 0:
            self._universalBTrans = (3.0 * N * Ti / summv2) ** 0.4
            self._universalBRot = 1.0 if sumIw2 == 0.0 else (rotDOF * Ti / sumIw2) ** 0.4
        else:
            self._universalBTrans = self._universalBRot = 1.0

    def getGlobalBetaTrans(self):
        return self._universalBTrans

    def getGlobalBetaRot(self):
        return self._universalBRot

    def getGlobalCurrentTemperature(self):
        return self._globalTemperature

    def getLocalSumIw2(self, thermostat=0):
        return self._local2KERot[thermostat]


class CellProcessor:
    """adapter/CellProcessor.h:29-94 — only the traversal-level hooks exist on the device path: the per-cell
    callbacks (processCell / processCellPair) are fused into one kernel launch per traversal."""

    def __init__(self, cutoffRadius, LJCutoffRadius):
        self._cutoffRadiusSquare = cutoffRadius * cutoffRadius
        self._LJCutoffRadiusSquare = LJCutoffRadius * LJCutoffRadius

    def getCutoffRadiusSquare(self):
        return self._cutoffRadiusSquare

    def getLJCutoffRadiusSquare(self):
        return self._LJCutoffRadiusSquare

    def initTraversal(self):
        raise NotImplementedError

    def endTraversal(self):
        raise NotImplementedError


class VectorizedCellProcessor(CellProcessor):
    """VectorizedCellProcessor(Domain&, cutoffRadius, LJcutoffRadius) — adapter/VectorizedCellProcessor.h:40-71."""

    def __init__(self, domain: Domain, cutoffRadius: float, LJcutoffRadius: float):
        super().__init__(cutoffRadius, LJcutoffRadius)
        self._domain = domain
        self._upot = 0.0
        self._virial = 0.0

    def initTraversal(self):
        self._upot = 0.0
        self._virial = 0.0

    def _accumulate(self, upot, virial):
        self._upot, self._virial = upot, virial

    def endTraversal(self):
        # VectorizedCellProcessor.cpp:155-156
        self._domain.setLocalVirial(self._virial)
        self._domain.setLocalUpot(self._upot)


class RDFCellProcessor(CellProcessor):
    """RDFCellProcessor(cutoffRadius, rdf) — adapter/RDFCellProcessor.h: the pair loops (RDFCellProcessor.cpp:18-133) are one
    sampling pass on the device (LinkedCells.traverseCells)."""

    def __init__(self, cutoffRadius: float, rdf: "RDF"):
        super().__init__(cutoffRadius, cutoffRadius)
        self._rdf = rdf

    def initTraversal(self):
        pass

    def endTraversal(self):
        pass


def _g5(x) -> str:
    """operator<< of a double at precision(5) (RDF.cpp:479): printf's %.5g; glibc writes a NaN with its sign"""
    x = float(x)
    if x != x:
        return "-nan" if np.signbit(x) else "nan"
    return "%.5g" % x


def _div(a, b) -> float:
    """IEEE division (the reference divides by counters that may be zero)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


class RDF:
    """The reference's RDF plugin (io/RDF.h, io/RDF.cpp) over the device histograms: constructor arguments = the nodes
    RDF::readXML reads (RDF.cpp:154-179); the numbers of sites come from the component set (RDF::init, RDF.cpp:35-151)."""

    def __init__(self, components: ComponentSet, cutoffRadius: float, *, writefrequency: int = 1, samplingfrequency: int = 1,
                 outputprefix: str = "mardyn", bins: int = 1, intervallength: float = 1.0, angularbins: int = 1,
                 initStatistics: int = 0):
        if angularbins > 1:
            raise NotImplementedError("angular RDF (angularbins > 1) is not sampled on the device")
        self._writeFrequency = int(writefrequency)
        self._samplingFrequency = int(samplingfrequency)
        self._outputPrefix = str(outputprefix)
        self._bins = int(bins)
        self._intervalLength = float(intervallength)
        self._initStatistics = int(initStatistics)
        self._numSites = [int(c.n_sites) for c in components.components]
        self._numberOfComponents = nC = len(self._numSites)
        self._doCollectSiteRDF = any(self._numSites[i] + self._numSites[j] > 2 for i in range(nC) for j in range(i, nC))
        self._cellProcessor = RDFCellProcessor(cutoffRadius, self)
        self._engine = None
        self._accumulatedNumberOfRDFTimesteps = 0
        self._globalAccumulatedCtr = np.zeros(nC, dtype=np.uint64)
        self._globalAccumulatedDistribution = np.zeros((nC * (nC + 1) // 2, self._bins), dtype=np.uint64)
        self._globalAccumulatedSiteDistribution = {p: np.zeros((self._numSites[p[0]], self._numSites[p[1]], self._bins), dtype=np.uint64)
                                                   for p in self._site_pairs()}
        self._zero_current()

    # component pair (i, j >= i) -> row of the molecule histogram, in the order of RDF::collectRDF (RDF.cpp:235-241)
    def _pair(self, i, j):
        nC = self._numberOfComponents
        return i * nC - (i * (i - 1)) // 2 + (j - i)

    def _site_pairs(self):
        nC, ns = self._numberOfComponents, self._numSites
        return [(i, j) for i in range(nC) for j in range(i, nC) if ns[i] + ns[j] > 2] if self._doCollectSiteRDF else []

    def _zero_current(self):
        nC = self._numberOfComponents
        self._numberOfRDFTimesteps = 0
        self._globalCtr = np.zeros(nC, dtype=np.uint64)
        self._distribution_global = np.zeros((nC * (nC + 1) // 2, self._bins), dtype=np.uint64)
        self._siteDistribution_global = {p: np.zeros((self._numSites[p[0]], self._numSites[p[1]], self._bins), dtype=np.uint64)
                                         for p in self._site_pairs()}

    def _configure(self, engine: DeviceEngine):
        if self._engine is not engine:
            engine.rdf_config(self._bins, self._intervalLength, self._doCollectSiteRDF)
            self._engine = engine

    def isEnabledSiteRDF(self):
        return self._doCollectSiteRDF

    # --- RDF::afterForces, RDF.cpp:573-581 (tickRDF and accumulateNumberOfMolecules are part of the device pass)
    def afterForces(self, particleContainer, domainDecomp, simstep: int):
        if simstep % self._samplingFrequency == 0 and simstep > self._initStatistics:
            self._numberOfRDFTimesteps += 1
            particleContainer.traverseCells(self._cellProcessor)

    # --- RDF::collectRDF, RDF.cpp:231-306: local counts of the device -> global values (summed over the ranks by a decomposition
    # that offers rdf_collect, decomp.py)
    def collectRDF(self, domainDecomp=None):
        if self._engine is None:
            return
        collect = getattr(domainDecomp, "rdf_collect", None)
        self.setGlobal(collect(self._engine) if collect else self._engine.rdf_read())

    def setGlobal(self, counts):
        """Global values of the current interval from a dict as DeviceEngine.rdf_read / decomp.rdf_collect return it."""
        self._numberOfRDFTimesteps = int(counts["samples"])
        self._globalCtr = np.asarray(counts["n_per_component"], dtype=np.uint64).copy()
        self._distribution_global = np.asarray(counts["mol"], dtype=np.uint64).reshape(-1, self._bins).copy()
        self._siteDistribution_global = {p: np.asarray(b, dtype=np.uint64).copy() for p, b in zip(self._site_pairs(), counts["site"])}

    # --- RDF::accumulateRDF, RDF.cpp:202-229
    def accumulateRDF(self):
        if self._numberOfRDFTimesteps <= 0:
            return
        self._accumulatedNumberOfRDFTimesteps += self._numberOfRDFTimesteps
        self._globalAccumulatedCtr += self._globalCtr
        self._globalAccumulatedDistribution += self._distribution_global
        for p, b in self._siteDistribution_global.items():
            self._globalAccumulatedSiteDistribution[p] += b

    # --- RDF::reset, RDF.cpp:309-340: everything but the accumulated values
    def reset(self):
        self._zero_current()
        if self._engine is not None:
            self._engine.rdf_reset()

    # --- RDF::endStep, RDF.cpp:343-375
    def endStep(self, particleContainer, domainDecomp, domain: Domain, simStep: int, directory: str = "."):
        import os

        if self._numberOfRDFTimesteps <= 0:
            return
        if simStep > 0 and simStep % self._writeFrequency == 0:
            self.collectRDF(domainDecomp)
            rank = domainDecomp.getRank() if hasattr(domainDecomp, "getRank") else 0
            if rank == 0:
                self.accumulateRDF()
                for i in range(self._numberOfComponents):
                    for j in range(i, self._numberOfComponents):
                        self.writeToFile(domain, os.path.join(directory, "%s_%d-%d.%09d.rdf" % (self._outputPrefix, i, j, simStep)), i, j)
            self.reset()

    # --- RDF::writeToFile, RDF.cpp:457-571
    def writeToFile(self, domain: Domain, filename: str, i: int, j: int):
        ni, nj = self._numSites[i], self._numSites[j]
        sites = ni + nj > 2
        V = domain.getGlobalVolume()
        nT, nA = self._numberOfRDFTimesteps, self._accumulatedNumberOfRDFTimesteps
        N_i = _div(int(self._globalCtr[i]), nT)
        N_Ai = _div(int(self._globalAccumulatedCtr[i]), nA)
        N_j = _div(int(self._globalCtr[j]), nT)
        N_Aj = _div(int(self._globalAccumulatedCtr[j]), nA)
        rho_i, rho_Ai, rho_j, rho_Aj = N_i / V, N_Ai / V, N_j / V, N_Aj / V
        out = ["# r\tcurr.{loc, int}\taccu.{loc, int}\t\tdV\tNpair(curr.)\tNpair(accu.)\t\tnorm(curr.)\tnorm(accu.)"]
        if sites:
            for m in range(ni):
                out.append("\t")
                for n in range(nj):
                    out.append("\t(%d, %d)_curr{loc, int}   (%d, %d)_accu{loc, int}" % (m, n, m, n))
        out.append("\n")
        out.append("# \n# ctr_i: %d\n# ctr_j: %d\n# V: %s\n# _universalRDFTimesteps: %d\n# _universalAccumulatedTimesteps: %d"
                   "\n# _samplingFrequency: %d\n# rho_i: %s (acc. %s)\n# rho_j: %s (acc. %s)\n# \n"
                   % (int(self._globalCtr[i]), int(self._globalCtr[j]), _g5(V), nT, nA, self._samplingFrequency, _g5(rho_i), _g5(rho_Ai),
                      _g5(rho_j), _g5(rho_Aj)))
        out.append("#r\trdf\trdf_{integral}\tacc_rdf acc_rdf_{integral}\t\tdV\tNpair(curr.)\tNpair(accu.)\t\tnormalization(curr.)\tnormalization(accu.)")
        if sites:
            for m in range(ni):
                out.append("\t")
                for n in range(nj):
                    out.append("\t(%d,%d)_curr{rdf, rdf_integral}   (%d,%d)_accu{rdf, rdf_integral}" % (m, n, m, n))
        out.append("\n")
        p = self._pair(i, j)
        dist, adist = self._distribution_global[p], self._globalAccumulatedDistribution[p]
        sdist = self._siteDistribution_global.get((i, j)) if sites else None
        sadist = self._globalAccumulatedSiteDistribution.get((i, j)) if sites else None
        Nsite_pair_int = np.zeros((ni, nj))
        Nsite_Apair_int = np.zeros((ni, nj))
        N_pair_int = N_Apair_int = 0.0
        w = self._intervalLength
        for l in range(self._bins):
            rmin, rmid, rmax = l * w, (l + 0.5) * w, (l + 1.0) * w
            r3min, r3max = rmin * rmin * rmin, rmax * rmax * rmax
            dV = (4.0 / 3.0) * np.pi * (r3max - r3min)
            N_pair = _div(int(dist[l]), nT)
            N_pair_int += N_pair
            N_Apair = _div(int(adist[l]), nA)
            N_Apair_int += N_Apair
            if i == j:
                N_pair_norm = 0.5 * N_i * (N_i - 1.0) * dV / V
                N_Apair_norm = 0.5 * N_Ai * (N_Ai - 1.0) * dV / V
                N_pair_int_norm = 0.5 * N_i * (N_i - 1.0) * 4.1887902 * r3max / V
                N_Apair_int_norm = 0.5 * N_Ai * (N_Ai - 1.0) * 4.1887902 * r3max / V
            else:
                N_pair_norm = N_i * N_j * dV / V
                N_Apair_norm = N_Ai * N_Aj * dV / V
                N_pair_int_norm = N_i * N_j * 4.1887902 * r3max / V
                N_Apair_int_norm = N_Ai * N_Aj * 4.1887902 * r3max / V
            out.append("%s\t%s %s\t%s %s\t\t%s\t%s\t%s\t\t%s\t%s" % (
                _g5(rmid), _g5(_div(N_pair, N_pair_norm)), _g5(_div(N_pair_int, N_pair_int_norm)), _g5(_div(N_Apair, N_Apair_norm)),
                _g5(_div(N_Apair_int, N_Apair_int_norm)), _g5(dV), _g5(N_pair), _g5(N_Apair), _g5(N_pair_norm), _g5(N_Apair_norm)))
            if sites:
                for m in range(ni):
                    out.append("\t")
                    for n in range(nj):
                        # the writer's factor 1/2 for the double count of same-component pairs with m != n (RDF.cpp:556-558)
                        cf = 0.5 if (i == j and m != n) else 1.0
                        ps = _div(cf * int(sdist[m, n, l]), nT)
                        Nsite_pair_int[m, n] += ps
                        ap = _div(cf * int(sadist[m, n, l]), nA)
                        Nsite_Apair_int[m, n] += ap
                        out.append("\t%s %s   %s %s" % (_g5(_div(ps, N_pair_norm)), _g5(_div(Nsite_pair_int[m, n], N_pair_int_norm)),
                                                        _g5(_div(ap, N_Apair_norm)), _g5(_div(Nsite_Apair_int[m, n], N_Apair_int_norm))))
            out.append("\n")
        with open(filename, "w") as f:
            f.write("".join(out))


def _g6(x) -> str:
    """operator<< of a double / long double at precision(6) (ofstream::precision(6) of every profile writer)"""
    x = float(x)
    if x != x:
        return "-nan" if np.signbit(x) else "nan"
    if np.isinf(x):
        return "-inf" if x < 0 else "inf"
    return "%.6g" % x


class SpatialProfile:
    """The reference's SpatialProfile plugin (plugins/SpatialProfile.{h,cpp}, plugins/profiles/*) over the device tables.
    Constructor arguments = the nodes SpatialProfile::readXML reads (SpatialProfile.cpp:22-134): mode ("cartesian" / "cylinder" or
    the LS1HIP_PROF_* value), units = (x, y, z) or (r, h, phi), writefrequency, init, recording, outputprefix, profiledComponent
    ("all" or the 1-based component id of the XML) and profiles = the names switched on among density, velocity, velocity3d,
    temperature, virial, virial2D; none given -> all (SpatialProfile.cpp:88-91).  The Virial2D writer does not exist here: its
    accumulators (density, DOF, kinetic, virial) are sampled, its file is not written."""

    CARTESIAN, CYLINDER = 0, 1

    def __init__(self, global_length, *, mode="cartesian", units=(1, 1, 1), writefrequency: int = 1, init: int = 0, recording: int = 1,
                 outputprefix: str = "profile", profiledComponent="all", profiles=()):
        if mode in ("cartesian", self.CARTESIAN):
            self._cylinder = False
        elif mode in ("cylinder", self.CYLINDER):
            self._cylinder = True
        else:
            raise ValueError("[SpatialProfile] Invalid mode. cylinder/cartesian")
        self._units = tuple(int(u) for u in units)
        self._writeFrequency, self._initStatistics, self._profileRecordingTimesteps = int(writefrequency), int(init), int(recording)
        self._outputPrefix = str(outputprefix)
        self._profiledComp = None if str(profiledComponent) == "all" else int(profiledComponent)  # 1-based, as in the XML
        known = ("density", "velocity", "velocity3d", "temperature", "virial", "virial2D")
        on = set(profiles)
        if on - set(known):
            raise ValueError("unknown profile(s): %s" % sorted(on - set(known)))
        self._ALL = not on  # "NO PROFILES SPECIFIED -> Outputting all"
        f = {k: (k in on) for k in known}
        # the profiles SpatialProfile::readXML adds (SpatialProfile.cpp:93-127)
        self._dens = f["density"] or f["velocity"] or f["velocity3d"] or f["virial"] or f["virial2D"] or self._ALL
        self._velAbs = f["velocity"] or self._ALL
        self._vel3d = f["velocity3d"] or self._ALL
        self._virial = f["virial"] or self._ALL
        self._temp = f["temperature"] or self._ALL
        self._dofkin = self._temp or f["virial2D"]
        # SpatialProfile::init (SpatialProfile.cpp:146-212)
        L = self._globalLength = np.asarray(global_length, dtype=np.float64).copy()
        u = self._units
        if self._cylinder:
            minXZ = min(L[0], L[2])
            R2max = .24 * minXZ * minXZ
            self._inv = (u[0] / R2max, u[1] / L[1], u[2] / (2 * np.pi))
            self._segmentVolume = np.pi / (self._inv[0] * self._inv[1] * u[2])
        else:
            self._inv = tuple(u[d] / L[d] for d in range(3))
            self._segmentVolume = L[0] * L[1] * L[2] / (u[0] * u[1] * u[2])
        self._uIDs = u[0] * u[1] * u[2]
        self._engine = None

    def quantities(self) -> int:
        """the LS1HIP_PROF_* mask of the enabled profiles"""
        E = DeviceEngine
        return ((E.PROF_VELOCITY if self._velAbs else 0) | (E.PROF_VELOCITY3D if self._vel3d else 0) |
                (E.PROF_TEMPERATURE if self._dofkin else 0) | (E.PROF_VIRIAL if self._virial else 0))

    def component(self) -> int:
        """0-based component id of ls1hip_profile_config (-1: all): componentid() == _profiledComp - 1 (SpatialProfile.cpp:244)"""
        return -1 if self._profiledComp is None else self._profiledComp - 1

    def attach(self, engine: DeviceEngine):
        """configure the device tables of `engine` for this plugin instance (one instance per engine)"""
        engine.profile_config(self.CYLINDER if self._cylinder else self.CARTESIAN, self._units, self.quantities(), self.component())
        self._engine = engine

    def samplesAt(self, simstep: int) -> bool:
        return simstep >= self._initStatistics and simstep % self._profileRecordingTimesteps == 0

    def writesAt(self, simstep: int) -> bool:
        return simstep >= self._initStatistics and simstep % self._writeFrequency == 0

    # --- SpatialProfile::endStep, SpatialProfile.cpp:233-328.  temperature: Domain::getCurrentTemperature(0) of this step, the value
    # from the kinetic sums BEFORE the thermostat scales (Domain.cpp:204-240; a row of ls1hip_run_log gives it).  sample = False:
    # the device loop has sampled already (ls1hip_run with profile_every / profile_from).
    def endStep(self, simstep: int, temperature: float, domainDecomp=None, directory: str = ".", sample: bool = True):
        if sample and self.samplesAt(simstep):
            self._engine.profile_sample()
        if self.writesAt(simstep):
            collect = getattr(domainDecomp, "profile_collect", None)
            tables = collect(self._engine) if collect else self._engine.profile_read()
            rank = domainDecomp.getRank() if hasattr(domainDecomp, "getRank") else 0
            if rank == 0:
                self.write(tables, simstep, temperature, directory)
            self._engine.profile_reset()

    def write(self, tables, simstep: int, temperature: float, directory: str = "."):
        import os

        for suffix, text in self.render(tables, simstep, temperature).items():
            with open(os.path.join(directory, "%s_%d%s" % (self._outputPrefix, simstep, suffix)), "w") as fh:
                fh.write(text)

    def render(self, tables, simstep: int, temperature: float):
        """{file suffix: text} of every writer, from global tables as DeviceEngine.profile_read / decomp.profile_collect return them"""
        acc = int(tables["samples"])
        out = {}
        if self._dens:
            out[".NDpr"] = self._file("the number density", "DensityProfile", ["//local density profile: Y - Z || X-projection\n"], tables, acc,
                                      lambda t, uID: [_div(float(t["n"][uID]), self._segmentVolume * acc)])
        if self._velAbs:
            out[".VAbspr"] = self._file("magnitude of velocity", "VelocityAbsProfile", ["//local velocity magnitude profile: Y - Z || X-projection\n"],
                                        tables, acc, lambda t, uID: [_div(t["vabs"][uID], int(t["n"][uID])) if int(t["n"][uID]) != 0 else 0.0])
        if self._vel3d:
            out[".V3Dpr"] = self._file("X-Y-Z components of velocity", "Velocity3dProfile",
                                       ["//local velocity component profile: Y - Z || X-projection\n"], tables, acc,
                                       lambda t, uID: [_div(t["v3"][uID][d], int(t["n"][uID])) if int(t["n"][uID]) != 0 else 0.0 for d in range(3)])
        if self._virial:
            out["_1D-Y.Vipr"] = self._virial_file(tables, acc, temperature)
        if self._temp:
            out[".Temppr"] = self._file("the temperature", "TemperatureProfile",
                                        ["//Temperature expressed by 2Ekin/#DOF\n", "//local temperature profile: Y - Z || X-projection\n"], tables, acc,
                                        lambda t, uID: [_div(t["ekin"][uID], int(t["dof"][uID])) if int(t["dof"][uID]) != 0 else 0.0])
        return out

    def _head(self, what, method, acc):
        local = "Local profile of " + what
        return ["//Segment volume: ", _g6(self._segmentVolume), "\n//Accumulated data sets: ", str(acc), "\n//", local,
                ". Output file generated by the \"", method, "\" method, plugins/profiles. \n"]

    def _dxyz(self):
        return ["// \t dX \t dY \t dZ \n", "\t", _g6(1 / self._inv[0]), "\t", _g6(1 / self._inv[1]), "\t", _g6(1 / self._inv[2]), "\n"]

    # --- <Profile>::output + ProfileBase::writeMatrix (DensityProfile.cpp:7-37, ProfileBase.cpp:8-73)
    def _file(self, what, method, lines, tables, acc, entry):
        out = self._head(what, method, acc) + lines + self._dxyz() + ["0 \t"]
        u, inv = self._units, self._inv
        if self._cylinder:  # ProfileBase::writeCylMatrix
            for r in range(u[0]):
                out += [_g6(0.5 * (np.sqrt(r + 1) + np.sqrt(r)) / np.sqrt(inv[0])), " \t"]
            out.append("\n")
            for h in range(u[1]):
                out += [_g6((h + 0.5) / inv[1]), "  \t"]
                for phi in range(u[2]):
                    for r in range(u[0]):
                        for x in entry(tables, h * u[0] * u[2] + r * u[2] + phi):
                            out += [_g6(x), "\t"]
                out.append("\n")
        else:  # ProfileBase::writeKartMatrix
            for z in range(u[2]):
                out += [_g6((z + 0.5) / inv[2]), "  \t"]
            out.append("\n")
            for y in range(u[1]):
                out += [_g6((y + 0.5) / inv[1]), "  \t"]
                for z in range(u[2]):
                    for x in range(u[0]):
                        for e in entry(tables, x * u[1] * u[2] + y * u[2] + z):
                            out += [_g6(e), "\t"]
                out.append("\n")
        return "".join(out)

    # --- VirialProfile::output (VirialProfile.cpp:7-96): the layer sums over the planes of constant y / h
    def _virial_file(self, tables, acc, globalTemperature):
        out = self._head("the partial pressures", "VirialProfile", acc) + self._dxyz() + ["0 \t\n", "# y\tvn-vt\tpx\tpy\tpz\n# \n"]
        u, L = self._units, self._globalLength
        layerHeight = L[1] / u[1]
        if self._cylinder:
            radius = L[0] / 2
            layerVolume = layerHeight * np.pi * radius * radius
        else:
            layerVolume = layerHeight * L[0] * L[2]
        ld = np.longdouble
        vi, n = tables["vi3"], tables["n"]
        for y in range(u[1]):
            hval = (y + 0.5) / self._inv[1]
            Px = Py = Pz = Ny = ld(0.0)
            for a in range(u[0]):
                for b in range(u[2]):
                    unID = y * u[0] * u[2] + a * u[2] + b if self._cylinder else a * u[1] * u[2] + y * u[2] + b
                    Px += ld(vi[unID][0])
                    Py += ld(vi[unID][1])
                    Pz += ld(vi[unID][2])
                    Ny += ld(int(n[unID]))
            Pd = Py - ld(.5) * (Px + Pz)
            with np.errstate(all="ignore"):
                den = ld(layerVolume * acc)
                T = ld(globalTemperature)
                out += [_g6(hval), "\t", _g6(Pd / den), "\t", _g6((T * Ny + Px) / den), "\t", _g6((T * Ny + Py) / den), "\t",
                        _g6((T * Ny + Pz) / den), "\n"]
        return "".join(out)


class LinkedCells:
    """Device-resident replacement of the reference's LinkedCells (seam B of SURVEY.md 8b).

    LinkedCells(bBoxMin, bBoxMax, cutoffRadius) as in particleContainer/LinkedCells.h; the extra keyword
    arguments carry what the reference takes from global_simulation (component set, LJ cutoff, device)."""

    def __init__(self, bBoxMin, bBoxMax, cutoffRadius, *, components: ComponentSet, globalLength=None,
                 LJCutoffRadius=None, device: int = 0, cellsInCutoffRadius: int = 1, my_rank: int = 0,
                 neighbor_rank=None, periodic: bool = True, engine: DeviceEngine | None = None):
        self._bmin = np.asarray(bBoxMin, dtype=np.float64).copy()
        self._bmax = np.asarray(bBoxMax, dtype=np.float64).copy()
        self._cutoffRadius = float(cutoffRadius)
        self.engine = engine or DeviceEngine(device)
        self.engine.set_components(components, cutoffRadius, LJCutoffRadius)
        self.engine.set_option("cells_in_cutoff", cellsInCutoffRadius)
        gl = self._bmax if globalLength is None else np.asarray(globalLength, dtype=np.float64)
        self.engine.set_domain(gl, self._bmin, self._bmax, my_rank, neighbor_rank, periodic)
        self._components = components

    # --- ParticleContainer.h:108-130
    def addParticles(self, ids, cid, r, v, q=None, D=None):
        self.engine.upload(ids, cid, r, v, q, D)

    # --- LinkedCells::update, LinkedCells.cpp:243-302
    def update(self):
        self.engine.rebin()

    # --- LinkedCells::updateMoleculeCaches, LinkedCells.cpp:1054-1086: the device SoA *is* the cache
    def updateMoleculeCaches(self):
        pass

    # --- LinkedCells::traverseCells, LinkedCells.cpp:564-575
    def traverseCells(self, cellProcessor: CellProcessor):
        if isinstance(cellProcessor, RDFCellProcessor):
            # the RDF traversal: one sampling pass over the same cells (histograms stay on the device until RDF::collectRDF)
            cellProcessor.initTraversal()
            cellProcessor._rdf._configure(self.engine)
            self.engine.rdf_sample()
            cellProcessor.endTraversal()
            return
        cellProcessor.initTraversal()
        cellProcessor._accumulate(*self.engine.forces(0))
        cellProcessor.endTraversal()

    # --- comm/compute overlap split, LinkedCells.cpp:577-609 (traversePartialInnermostCells / NonInnermost)
    def traversePartialInnermostCells(self, cellProcessor, stage: int, stageCount: int):
        if stage == 0:
            cellProcessor.initTraversal()
            self.engine.forces(1, want_macro=False)

    def traverseNonInnermostCells(self, cellProcessor):
        cellProcessor._accumulate(*self.engine.forces(2))
        cellProcessor.endTraversal()

    # --- LinkedCells::deleteOuterParticles, LinkedCells.cpp:611-628: halo copies live in their own segment and
    # are rebuilt by the next exchange; nothing to delete.
    def deleteOuterParticles(self):
        pass

    def requiresForceExchange(self):
        return False  # full-shell: C08CellPairTraversal.h:35

    def getNumberOfParticles(self):
        return self.engine.count()[0]

    def getCutoff(self):
        return self._cutoffRadius

    def getBoundingBoxMin(self, d):
        return float(self._bmin[d])

    def getBoundingBoxMax(self, d):
        return float(self._bmax[d])

    def getCellLength(self):
        return self.engine.grid()[1]

    def get_halo_L(self, d):
        dims, clen, hw = self.engine.grid()
        return float(clen[d] * hw)

    # host views (the reference's iterator(ONLY_INNER_AND_BOUNDARY) read access)
    def molecules(self):
        return self.engine.download_state()

    def forces(self, with_vi=False):
        return self.engine.download_forces(with_vi)


class DomainDecompBase:
    """Sequential periodic boundary: parallel/DomainDecompBase.cpp:51-86."""

    def balanceAndExchange(self, lastTraversalTime, forceRebalancing, moleculeContainer: LinkedCells, domain):
        self.exchangeMolecules(moleculeContainer, domain)

    def exchangeMolecules(self, moleculeContainer: LinkedCells, domain):
        # leaving molecules were wrapped by update(); populate the halo layer with copies
        moleculeContainer.engine.halo()

    def getBoundingBoxMin(self, d, domain):
        return 0.0

    def getBoundingBoxMax(self, d, domain):
        return domain.getGlobalLength(d)


class Integrator:
    def __init__(self, timestepLength=0.0):
        self._timestepLength = float(timestepLength)

    def getTimestepLength(self):
        return self._timestepLength

    def setTimestepLength(self, dt):
        self._timestepLength = float(dt)


class Leapfrog(Integrator):
    """integrators/Leapfrog.cpp:17-150 — same three-state machine."""

    STATE_UNKNOWN, STATE_NEW_TIMESTEP, STATE_PRE_FORCE_CALCULATION, STATE_POST_FORCE_CALCULATION = 0, 1, 2, 3

    def __init__(self, timestepLength=0.0):
        super().__init__(timestepLength)
        self.init()

    def init(self):
        self._state = self.STATE_POST_FORCE_CALCULATION

    def eventNewTimestep(self, molCont: LinkedCells, domain: Domain):
        if self._state == self.STATE_POST_FORCE_CALCULATION:
            self._state = self.STATE_NEW_TIMESTEP  # transition3to1
            molCont.engine.kick_drift(self._timestepLength)  # transition1to2 -> upd_preF
            self._state = self.STATE_PRE_FORCE_CALCULATION

    def eventForcesCalculated(self, molCont: LinkedCells, domain: Domain):
        if self._state == self.STATE_PRE_FORCE_CALCULATION:
            summv2, sumIw2, N, rotDOF = molCont.engine.kick(0.5 * self._timestepLength)  # transition2to3 -> upd_postF
            domain.setLocalSummv2(summv2, 0)
            domain.setLocalSumIw2(sumIw2, 0)
            domain.setLocalNrotDOF(0, N, rotDOF)
            self._state = self.STATE_POST_FORCE_CALCULATION


class VelocityScalingThermostat:
    """thermostats/VelocityScalingThermostat.cpp:9-96, global (non component-wise) branch."""

    def __init__(self):
        self._globalBetaTrans = 1.0
        self._globalBetaRot = 1.0

    def setGlobalBetaTrans(self, beta):
        self._globalBetaTrans = float(beta)

    def setGlobalBetaRot(self, beta):
        self._globalBetaRot = float(beta)

    def apply(self, moleculeContainer: LinkedCells):
        moleculeContainer.engine.scale_velocities(self._globalBetaTrans, self._globalBetaRot)


def simulate(container: LinkedCells, decomp: DomainDecompBase, cellProcessor: VectorizedCellProcessor,
             integrator: Leapfrog, domain: Domain, nsteps: int, initial_forces: bool = True,
             thermostat: VelocityScalingThermostat | None = None):
    """The hot-path part of Simulation::prepare_start / simulate (Simulation.cpp:813-892, 979-1167), call for call."""
    if initial_forces:
        container.update()
        decomp.balanceAndExchange(1.0, False, container, domain)
        container.updateMoleculeCaches()
        container.traverseCells(cellProcessor)
        container.deleteOuterParticles()
    for _ in range(nsteps):
        integrator.eventNewTimestep(container, domain)
        container.update()
        decomp.balanceAndExchange(0.0, False, container, domain)
        container.updateMoleculeCaches()
        container.traverseCells(cellProcessor)
        container.deleteOuterParticles()
        integrator.eventForcesCalculated(container, domain)
        if thermostat is not None:  # Simulation.cpp:1099-1131
            domain.calculateGlobalValues(decomp, container, True, 1.0)
            thermostat.setGlobalBetaTrans(domain.getGlobalBetaTrans())
            thermostat.setGlobalBetaRot(domain.getGlobalBetaRot())
            thermostat.apply(container)
