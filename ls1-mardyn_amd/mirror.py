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

import os

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


class ODFCellProcessor(CellProcessor):
    """ODFCellProcessor(cutoffRadius, odf) — adapter/ODFCellProcessor.h: the pair loops (ODFCellProcessor.cpp:16-81) are one sampling
    pass on the device (LinkedCells.traverseCells)."""

    def __init__(self, cutoffRadius: float, odf: "ODF"):
        super().__init__(cutoffRadius, cutoffRadius)
        self._odf = odf


_ODF_NOTE = ("//The output is to be interpreted as follows: an orientation with a value of ODF_normed = 1 has the same probability as "
             "random orientation. ODF_normed = 1.4 means 40% higher probability than random orientation, 0.4 means 60% lower "
             "probability than random orientation etc.\n")


class ODF:
    """The reference's ODF plugin (io/ODF.h, io/ODF.cpp) over the device arrays: keyword arguments = the nodes ODF::readXML reads
    (ODF.cpp:6-24); the pairings come from the component set (ODF::init, ODF.cpp:26-79)."""

    def __init__(self, components: ComponentSet, cutoffRadius: float, *, writefrequency: int = 1, initstatistics: int = 0,
                 recordingtimesteps: int = 1, outputprefix: str = "mardyn", phi1increments: int = 1, phi2increments: int = 1,
                 gammaincrements: int = 1, shellcutoff: float = 1.0):
        self._writeFrequency = int(writefrequency)
        self._initStatistics = int(initstatistics)
        self._recordingTimesteps = int(recordingtimesteps)
        self._outputPrefix = str(outputprefix)
        self._phi1Increments, self._phi2Increments = int(phi1increments), int(phi2increments)
        self._gammaIncrements = int(gammaincrements)
        self._shellCutOff = float(shellcutoff)
        numDipolar = sum(1 for c in components.components if len(c.dipoles) == 1)
        self._numPairs = numDipolar * numDipolar
        self._numElements = self._phi1Increments * self._phi2Increments * self._gammaIncrements + 1
        self._cellProcessor = ODFCellProcessor(cutoffRadius, self)
        self._engine = None
        self._readStartingStep = False
        self._ODF = np.zeros((2, 2, self._numElements), dtype=np.uint64)  # [a][b] = _ODF<a+1><b+1>

    def _configure(self, engine: DeviceEngine):
        if self._engine is not engine:
            engine.odf_config(self._phi1Increments, self._phi2Increments, self._gammaIncrements, self._shellCutOff)
            self._engine = engine

    # --- ODF::afterForces, ODF.cpp:81-85
    def afterForces(self, particleContainer, domainDecomp, simstep: int):
        if simstep > self._initStatistics and simstep % self._recordingTimesteps == 0:
            particleContainer.traverseCells(self._cellProcessor)

    # --- ODF::collect, ODF.cpp:333-384: local counts of the device -> global values (summed over the ranks by a decomposition
    # that offers odf_collect, decomp.py)
    def collect(self, domainDecomp=None):
        if self._engine is None:
            return
        collect = getattr(domainDecomp, "odf_collect", None)
        self.setGlobal((collect(self._engine) if collect else self._engine.odf_read())["hist"])

    def setGlobal(self, hist):
        """Global arrays [2, 2, W] as DeviceEngine.odf_read / decomp.odf_collect return them under "hist"."""
        self._ODF = np.asarray(hist, dtype=np.uint64).reshape(2, 2, self._numElements).copy()

    # --- ODF::reset, ODF.cpp:104-121
    def reset(self):
        self._ODF[:] = 0
        if self._engine is not None:
            self._engine.odf_reset()

    # --- ODF::endStep, ODF.cpp:87-102: nothing at the first call (a resumed run would overwrite the last file of the previous one)
    def endStep(self, particleContainer, domainDecomp, domain, simstep: int, directory: str = "."):
        if not self._readStartingStep:
            self._readStartingStep = True
            return
        if simstep > self._initStatistics and simstep % self._writeFrequency == 0:
            self.collect(domainDecomp)
            if (domainDecomp.getRank() if hasattr(domainDecomp, "getRank") else 0) == 0:
                self.output(domain, simstep, directory)
            self.reset()

    # --- ODF::output, ODF.cpp:386-506: one file for one dipolar component (the array 11 whatever the id of that component: a lone
    # single-dipole component with id 1 counts into 22 and leaves .ODF11 without counts), four files otherwise
    def output(self, domain, timestep: int, directory: str = "."):
        import os

        P1, P2, G, W = self._phi1Increments, self._phi2Increments, self._gammaIncrements, self._numElements
        prefix = os.path.join(directory, "%s%07d" % (self._outputPrefix, timestep))
        head = "//Output generated by ODF plugin\n" + _ODF_NOTE + "//Angular distribution at time step = %d for component pairing pairing " % timestep
        if self._numPairs == 1:
            files = [("11", (0, 0), "11\n", "cosPhi1\tcosPhi2\tGamma12\tODF_normed\n")]
            prec = 6
        else:
            cos = "cosPhi1\tcosPhi2\tcosGamma12\tODF_normed\n"
            files = [("11", (0, 0), "11.\n", cos), ("12", (0, 1), "12\n", cos), ("22", (1, 1), "22\n", "phi1\tphi2\tgamm12\tODF_normed\n"),
                     ("21", (1, 0), "21\n", cos)]
            prec = 5
        fmt = lambda x: ("-nan" if np.signbit(x) else "nan") if x != x else "%.*g" % (prec, x)  # noqa: E731  operator<< at precision(prec)
        rows = []
        cosPhi1, cosPhi2, Gamma12 = 1. + 1. / P1, 1. - 2. / P2, 0.
        for i in range(W - 1):
            Gamma12 += np.pi / G
            if i % G == 0:
                cosPhi2 -= 2. / P2
                Gamma12 = 0.5 * np.pi / G
            if i % (G * P2) == 0:
                cosPhi1 -= 2. / P1
                cosPhi2 = 1. - 1. / P2
            rows.append("%s\t%s\t%s\t" % (fmt(cosPhi1), fmt(cosPhi2), fmt(Gamma12)))
        names = []
        for tag, (a, b), end, columns in files:
            h = self._ODF[a, b]
            average = float(h[1:].astype(np.float64).sum()) / (float(W) - 1.)
            with open(prefix + ".ODF" + tag, "w") as fh:
                fh.write(head + end + columns)
                fh.write("".join(r + fmt(_div(float(h[i + 1]), average)) + "\n" for i, r in enumerate(rows)))
            names.append(prefix + ".ODF" + tag)
        return names


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


class ARDF(RDF):
    """The RDF plugin with <angularbins> > 1 (RDF.cpp:49-55): molecule histogram, counters and the angular histograms
    [c_central][c_other][b * A + a] of ONE device traversal; site histograms are off.  endStep writes the .ardf files of every
    ordered component pair (RDF.cpp:361-370); the .rdf files stay with mirror.RDF."""

    def __init__(self, components: ComponentSet, cutoffRadius: float, *, bins: int = 1, intervallength: float = 1.0, angularbins: int = 2,
                 writefrequency: int = 1, samplingfrequency: int = 1, outputprefix: str = "mardyn"):
        if angularbins <= 1:
            raise ValueError("angularbins must be > 1 (mirror.RDF is the plugin without the angular part)")
        self._angularBins = int(angularbins)
        self._angularIntervalLength = 2. / self._angularBins
        super().__init__(components, cutoffRadius, writefrequency=writefrequency, samplingfrequency=samplingfrequency,
                         outputprefix=outputprefix, bins=bins, intervallength=intervallength)
        self._doCollectSiteRDF = False
        self._globalAccumulatedSiteDistribution = {}
        nC = self._numberOfComponents
        self._globalAccumulatedARDFDistribution = np.zeros((nC, nC, self._bins * self._angularBins), dtype=np.uint64)
        self._zero_current()

    def _zero_current(self):
        super()._zero_current()
        nC = self._numberOfComponents
        self._ARDFdistribution_global = np.zeros((nC, nC, self._bins * self._angularBins), dtype=np.uint64)

    def _configure(self, engine: DeviceEngine):
        if self._engine is not engine:
            engine.rdf_config(self._bins, self._intervalLength, False)
            engine.rdf_config_angular(self._angularBins)
            self._engine = engine

    def setGlobal(self, counts):
        super().setGlobal(counts)
        nC = self._numberOfComponents
        self._ARDFdistribution_global = np.asarray(counts["ardf"], dtype=np.uint64).reshape(nC, nC, -1).copy()

    # --- RDF::accumulateRDF, RDF.cpp:221-228
    def accumulateRDF(self):
        if self._numberOfRDFTimesteps <= 0:
            return
        super().accumulateRDF()
        self._globalAccumulatedARDFDistribution += self._ARDFdistribution_global

    def endStep(self, particleContainer, domainDecomp, domain: Domain, simStep: int, directory: str = "."):
        import os

        if self._numberOfRDFTimesteps <= 0:
            return
        if simStep > 0 and simStep % self._writeFrequency == 0:
            self.collectRDF(domainDecomp)
            if (domainDecomp.getRank() if hasattr(domainDecomp, "getRank") else 0) == 0:
                self.accumulateRDF()
                for i in range(self._numberOfComponents):
                    for j in range(self._numberOfComponents):
                        self.writeToFileARDF(domain, os.path.join(directory, "%s_%d-%d.%09d.ardf" % (self._outputPrefix, i, j, simStep)), i, j)
            self.reset()

    # --- RDF::writeToFileARDF, RDF.cpp:377-453 (the stream keeps its default precision of 6)
    def writeToFileARDF(self, domain: Domain, filename: str, i: int, j: int):
        V = domain.getGlobalVolume()
        nT, nA = self._numberOfRDFTimesteps, self._accumulatedNumberOfRDFTimesteps
        N_i, N_Ai = _div(int(self._globalCtr[i]), nT), _div(int(self._globalAccumulatedCtr[i]), nA)
        N_j, N_Aj = _div(int(self._globalCtr[j]), nT), _div(int(self._globalAccumulatedCtr[j]), nA)
        out = ["\n# \n# ctr_i: %d\n# ctr_j: %d\n# V: %s\n# _universalRDFTimesteps: %d\n# _universalAccumulatedTimesteps: %d"
               "\n# _samplingFrequency: %d\n# rho_i: %s (acc. %s)\n# rho_j: %s (acc. %s)\n# \n"
               % (int(self._globalCtr[i]), int(self._globalCtr[j]), _g6(V), nT, nA, self._samplingFrequency, _g6(N_i / V), _g6(N_Ai / V),
                  _g6(N_j / V), _g6(N_Aj / V)),
               "#r\tcos(phi)\tcounter\tardf\tardf_{integral}\tacc_rdf acc_rdf_{integral}\t\tdV\tNpair(curr.)\tNpair(accu.)\t\t"
               "normalization(curr.)\tnormalization(accu.)\n"]
        cur, acc = self._ARDFdistribution_global[i, j], self._globalAccumulatedARDFDistribution[i, j]
        same = (N_i * (N_i - 1.0), N_Ai * (N_Ai - 1.0)) if i == j else (N_i * N_j, N_Ai * N_Aj)
        w, aw, A = self._intervalLength, self._angularIntervalLength, self._angularBins
        N_pair_int = N_Apair_int = 0.0
        for l in range(self._bins * A):
            radialID, angularID = divmod(l, A)
            rmin, rmid, rmax = radialID * w, (radialID + 0.5) * w, (radialID + 1.0) * w
            cosPhiMin, cosPhiMid, cosPhiMax = 1. - angularID * aw, 1. - (angularID + 0.5) * aw, 1. - (angularID + 1.0) * aw
            r3min, r3max = rmin * rmin * rmin, rmax * rmax * rmax
            dV = 2. / 3. * np.pi * ((r3max - r3min) * (1. - cosPhiMax) + (r3min - r3max) * (1. - cosPhiMin))
            N_pair = _div(int(cur[l]), nT)
            N_pair_int += N_pair
            N_Apair = _div(int(acc[l]), nA)
            N_Apair_int += N_Apair
            cone = r3min + 0.5 * ((r3max - r3min) * (1 - cosPhiMax))
            N_pair_norm, N_Apair_norm = same[0] * dV / V, same[1] * dV / V
            N_pair_int_norm, N_Apair_int_norm = same[0] * 4.1887902 * cone / V, same[1] * 4.1887902 * cone / V
            out.append("%s\t%s\t%d\t%s %s\t%s %s\t\t%s\t%s\t%s\t\t%s\t%s\n" % (
                _g6(rmid), _g6(cosPhiMid), int(cur[l]), _g6(_div(N_pair, N_pair_norm)), _g6(_div(N_pair_int, N_pair_int_norm)),
                _g6(_div(N_Apair, N_Apair_norm)), _g6(_div(N_Apair_int, N_Apair_int_norm)), _g6(dV), _g6(N_pair), _g6(N_Apair),
                _g6(N_pair_norm), _g6(N_Apair_norm)))
        with open(filename, "w") as f:
            f.write("".join(out))


class CavityWriter:
    """The reference's CavityWriter plugin (io/CavityWriter.{h,cpp}) over the device pass: keyword arguments = the nodes
    CavityWriter::readXML reads (CavityWriter.cpp:18-111); ControlVolume = (x0, x1, y0, y1, z0, z1) or None (the whole domain);
    componentid: the ids that name the output files (every molecule counts whatever its component).  numTimesteps: the run length
    the incremental file numbers are sized by (Simulation::getNumTimesteps); initStatistics: Simulation::getInitStatistics."""

    _ELEMENT = ("C ", "N ", "O ", "F ")  # by component id, "Ne " above (CavityWriter.cpp:223-227)

    def __init__(self, length, *, writefrequency: int = 1, outputprefix: str = "mardyn", incremental: int = 1, maxNeighbours: int,
                 radius: float, Nx: int, Ny: int, Nz: int, ControlVolume=None, componentid=(0,), numTimesteps: int = 1,
                 initStatistics: int = 0):
        self._length = np.asarray(length, dtype=np.float64).reshape(3)
        self._writeFrequency, self._outputPrefix, self._incremental = int(writefrequency), str(outputprefix), int(incremental) != 0
        self._maxNeighbors, self._radius = int(maxNeighbours), float(np.float32(radius))
        self._N = (int(Nx), int(Ny), int(Nz))
        cv = (0., self._length[0], 0., self._length[1], 0., self._length[2]) if ControlVolume is None else ControlVolume
        self._controlVolume = tuple(float(v) for v in cv)
        self._componentids = sorted(set(int(k) for k in componentid))  # a std::map: ascending ids
        self._numTimesteps, self._initStatistics = int(numTimesteps), int(initStatistics)
        self._engine = None
        self._pieces = []  # (lo, n, flags [n0, n1, n2]) of every rank, in rank order: the active sets
        self._numCavities = 0

    # --- CavityWriter::init, CavityWriter.cpp:113-146
    def init(self, engine: DeviceEngine):
        cv = self._controlVolume
        engine.cavity_config(*self._N, self._maxNeighbors, self._radius, cv[0::2], cv[1::2])
        self._engine = engine

    # --- CavityWriter::afterForces, CavityWriter.cpp:160-174: cavityStep + communicateNumCavities
    def afterForces(self, particleContainer, domainDecomp, simstep: int):
        if simstep >= self._initStatistics and simstep % self._writeFrequency == 0:
            self._engine.cavity_sample()
            collect = getattr(domainDecomp, "cavity_collect", None)
            self.setGlobal(collect(self._engine, self._N) if collect else self._engine.cavity_read())

    def setGlobal(self, res):
        """The active sets from DeviceEngine.cavity_read (one rank) or decomp.cavity_collect (pieces of all ranks, global n_active)."""
        self._pieces = list(res.get("pieces") or [(res["lo"], res["n"], res["flags"])])
        self._numCavities = int(res["n_active"])

    def nodePositions(self):
        """tq of every node (CavityEnsemble.cpp:158-171): float64 [Nx, Ny, Nz, 3]."""
        cv = self._controlVolume
        ax = [cv[2 * d] + (0.5009756 + np.arange(self._N[d])) * ((cv[2 * d + 1] - cv[2 * d]) / float(self._N[d])) for d in range(3)]
        return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)

    def fileName(self, cid: int, simstep: int) -> str:
        name = "%s-c%d" % (self._outputPrefix, cid)
        if self._incremental:
            # (int) ceil(log(double(numTimesteps / _writeFrequency)) / log(10.)), aligned_number (CavityWriter.cpp:188-193)
            num_digits = int(np.ceil(_div(np.log(float(self._numTimesteps // self._writeFrequency)), np.log(10.))))
            name += "-" + "%0*d" % (max(num_digits, 0), simstep // self._writeFrequency)
        return name + ".cav.xyz"

    def render(self, cid: int) -> str:
        """The text of one file: the global number of cavities, "comment line", then rank by rank (CavityWriter.cpp:211-235) one line
        per active node in ascending tid (z fastest)."""
        el = self._ELEMENT[cid] if 0 <= cid < 4 else "Ne "
        pos, out = self.nodePositions(), ["%d\ncomment line\n" % self._numCavities]
        for lo, n, flags in self._pieces:
            r = pos[lo[0]:lo[0] + n[0], lo[1]:lo[1] + n[1], lo[2]:lo[2] + n[2]][np.asarray(flags).reshape(tuple(n)) != 0]
            out += ["%s%s\t%s\t%s\n" % (el, _g6(p[0]), _g6(p[1]), _g6(p[2])) for p in r]
        return "".join(out)

    # --- CavityWriter::endStep, CavityWriter.cpp:176-237: writes whenever simstep % _writeFrequency == 0, also before initStatistics
    # (the active set is then whatever it was)
    def endStep(self, particleContainer, domainDecomp, domain, simstep: int, directory: str = "."):
        if simstep % self._writeFrequency != 0:
            return []
        names = []
        if (domainDecomp.getRank() if hasattr(domainDecomp, "getRank") else 0) == 0:
            for cid in self._componentids:
                names.append(os.path.join(directory, self.fileName(cid, simstep)))
                with open(names[-1], "w") as fh:
                    fh.write(self.render(cid))
        return names


class Planar:
    """The reference's planar long-range correction (longRange/Planar.{h,cpp}) over the device tables: readXML-style arguments
    (slabs, frequency, region = (left, right) with right = "box" allowed, writecontrol start / frequency / stop), calculateLongRange
    = one ls1hip_long_range_planar, writeProfiles = the LRC_TS%09d.dat writer (Planar.cpp:1110-1162)."""

    def __init__(self, length, slabs: int = 10, frequency: int = 10, region=None, temperature: float = 0.0, start: int = 1,
                 writefrequency: int = 10, stop: int = 100):
        if writefrequency < 1 or stop <= start:
            raise ValueError("writecontrol: frequency >= 1 and stop > start (Planar.cpp:196-205)")
        self._ymax = float(np.asarray(length, dtype=np.float64)[1])
        left, right = (0.0, self._ymax) if region is None else region
        self._region = (float(left), self._ymax if right == "box" else float(right))
        self._slabs, self._frequency, self._temperature = int(slabs), int(frequency), float(temperature)
        self._write = (int(start), int(writefrequency), int(stop))
        self._engine = None

    def init(self, engine):
        engine.planar_config(self._slabs, self._frequency, self._region, self._temperature)
        self._engine = engine

    def calculateLongRange(self, domain=None):
        up, vir = self._engine.planar()
        if domain is not None and hasattr(domain, "setUpotCorr"):
            domain.setUpotCorr(up)
            domain.setVirialCorr(vir)
        return up, vir

    def render(self, tables) -> str:
        """the text of one file from tables as DeviceEngine.planar_read returns them (rho, f, u: [LJ rows, slabs])"""
        rho, f, u = (np.asarray(tables[k], dtype=np.float64) for k in ("rho", "f", "u"))
        rows, slabs = rho.shape
        sci = lambda x: "%24s" % ("%.15e" % x)  # noqa: E731  FORMAT_SCI_MAX_DIGITS
        out = ["                     pos"] + ["            rho_l_LRC[%d]                F_LRC[%d]                u_LRC[%d]" % (k, k, k) for k in range(rows)] + ["\n"]
        per = self._ymax / slabs
        for pi in range(slabs):
            pos = per * (pi + 0.5)
            # (the first position is written before any FORMAT_SCI_MAX_DIGITS: default notation; the flags stay set afterwards)
            out.append("%24s" % _g6(pos) if pi == 0 else sci(pos))
            inside = self._region[0] <= pos <= self._region[1]
            for k in range(rows):
                out += [sci(rho[k, pi]), sci(f[k, pi] if inside else 0.0), sci(u[k, pi])]
            out.append("\n")
        return "".join(out)

    def writeProfiles(self, simstep: int, directory: str = ".", tables=None):
        start, freq, stop = self._write
        if simstep % freq != 0 or simstep < start or simstep > stop:
            return None
        path = os.path.join(directory, "LRC_TS%09d.dat" % simstep)
        with open(path, "w") as fh:
            fh.write(self.render(self._engine.planar_read() if tables is None else tables))
        return path


class WallPotential:
    """The reference's plugin WallPotential (plugins/WallPotential.{h,cpp}) over the device pass: the XML's parameters by their names —
    potential (93 | 104), density, sigma, epsilon, yoff, ycut, width, delta — and components = {cid (1-based, the XML's @id): (xi, eta)}.
    As in readXML (:43-75) an empty `components` makes EVERY component feel the wall, with xi = eta = 0 (so with no force)."""

    def __init__(self, potential: int = 93, density: float = 1.0, sigma: float = 1.0, epsilon: float = 1.0, yoff: float = 0.0,
                 ycut: float = 1.0, width: float = 0.0, delta: float = 0.0, components=None):
        if int(potential) not in (93, 104):
            raise ValueError(f"potential must be 93 or 104, got {potential} (the reference falls back to 93 with a log line)")
        self.potential, self.density, self.sigma, self.epsilon = int(potential), float(density), float(sigma), float(epsilon)
        self.yoff, self.ycut, self.width, self.delta = float(yoff), float(ycut), float(width), float(delta)
        self.components = {int(k): (float(xi), float(eta)) for k, (xi, eta) in (components or {}).items()}
        self._engine = None

    def arrays(self, ncomp: int):
        """consider [ncomp], xi [ncomp], eta [ncomp] as ls1hip_wall_config takes them"""
        consider = np.ones(ncomp, dtype=np.int32) if not self.components else np.zeros(ncomp, dtype=np.int32)
        xi, eta = np.zeros(ncomp), np.zeros(ncomp)
        for k, (x, e) in self.components.items():
            if not 1 <= k <= ncomp:
                raise ValueError(f"component id {k} outside 1..{ncomp}")
            consider[k - 1], xi[k - 1], eta[k - 1] = 1, x, e
        return consider, xi, eta

    def init(self, engine):
        engine.wall_config(self.potential, self.density, self.sigma, self.epsilon, self.yoff, self.ycut, self.width, self.delta,
                           *self.arrays(len(engine.n_sites)))
        self._engine = engine

    def siteWiseForces(self, simstep: int = 1):
        """one pass on the engine's current forces (wall AND configured mirrors: they share the pass); nothing at simstep 0 (:354)"""
        return None if simstep == 0 else self._engine.wall_apply()


class Mirror:
    """The reference's plugin Mirror (plugins/Mirror.{h,cpp}), types MT_REFLECT (1) and MT_FORCE_CONSTANT (2): type, dir ('|-o' left,
    'o-|' right) or direction (0 | 1), coord (position/coord), refID (position/refID), cid (0 all, else 1-based), forceConstant.
    slot: which of the device's 4 mirrors this one is."""
    REFUSED = {3: "MT_ZERO_GRADIENT is deprecated", 4: "MT_NORMDISTR_MB is deprecated",
               5: "MT_MELAND_2004 deletes molecules and draws random numbers", 6: "MT_RAMPING deletes molecules and draws random numbers"}

    def __init__(self, type: int = 1, dir: str | None = None, direction: int = 0, coord: float = 0.0, refID: int = 0, cid: int = 0,  # noqa: A002
                 forceConstant: float = 100.0, slot: int = 0):
        if int(type) in self.REFUSED:
            raise NotImplementedError(f"mirror type {type}: {self.REFUSED[int(type)]}; not applied on the device")
        if int(type) not in (1, 2):
            raise ValueError(f"mirror type must be 1 (MT_REFLECT) or 2 (MT_FORCE_CONSTANT), got {type}")
        if int(refID) != 0:
            raise NotImplementedError("position/refID != 0 (a position tracked by DistControl) is not served on the device")
        if dir is not None and dir not in ("|-o", "o-|"):
            raise ValueError(f"dir must be '|-o' or 'o-|', got {dir!r}")
        self.type, self.cid, self.coord, self.forceConstant, self.slot = int(type), int(cid), float(coord), float(forceConstant), int(slot)
        self.direction = int(direction) if dir is None else int(dir == "o-|")  # (@dir overrides <direction>, Mirror.cpp:94-102)
        self._engine = None

    def init(self, engine):
        engine.mirror_config(self.slot, self.type, self.direction, self.coord, self.cid, self.forceConstant)
        self._engine = engine

    def afterForces(self):
        """one pass on the engine's current forces and velocities (every configured mirror AND a configured wall: they share the pass)"""
        return self._engine.wall_apply()


class TemperatureControl:
    """The reference's region-wise thermostat (thermostats/TemperatureControl.{h,cpp}, method VelocityScaling) over the device passes:
    readXML-style arguments (control start / frequency / stop; per region a dict with lc, uc ('box' allowed per coordinate),
    temperature, component, numslabs, exponent, directions, writefreq, fileprefix and optionally ramp = dict(start, end, update_start,
    update_stop, update_freq)), DoLoopsOverMolecules = one ls1hip_temperature_control, write = the beta_log writer.  Inside
    ls1hip_run the device does the control itself; call ramp(simstep) / write(simstep) between runs."""

    def __init__(self, length, start: int = 0, frequency: int = 1, stop: int = 2 ** 63 - 1, regions=()):
        L = np.asarray(length, dtype=np.float64)
        self._control = (int(start), int(frequency), int(stop))
        self._regions = []
        for r in regions:
            uc = [L[d] if u == "box" else float(u) for d, u in enumerate(r["uc"])]
            ramp = r.get("ramp")
            if ramp:  # TemperatureControl.cpp:142-152
                ramp = dict(ramp, elapsed=0, slope=(ramp["end"] - ramp["start"]) / (ramp["update_stop"] - ramp["update_start"]))
            writefreq = int(r.get("writefreq", 1000)) or 1000  # 0 is reset to 1000 (:208-213)
            self._regions.append(dict(lc=[float(x) for x in r["lc"]], uc=uc, temperature=float(r["temperature"]), component=int(r.get("component", 0)),
                                      numslabs=int(r.get("numslabs", 1)), exponent=float(r.get("exponent", 0.0)), directions=r.get("directions", "xyz"),
                                      writefreq=writefreq, fileprefix=r.get("fileprefix", "beta_log"), ramp=ramp))
        self._engine = None

    def _measures(self, simstep: int) -> bool:
        start, freq, stop = self._control
        return simstep % freq == 0 and start <= simstep < stop

    def init(self, engine, directory: str | None = None):
        """configure the device; with a directory also InitBetaLogfile (TemperatureControl.cpp:435-453): the 8-byte write frequency"""
        engine.tempcontrol_config(*self._control)
        for k, r in enumerate(self._regions):
            rid = engine.tempcontrol_region(r["lc"], r["uc"], r["temperature"], r["component"], r["numslabs"], r["exponent"], r["directions"])
            assert rid == k + 1
            if directory is not None:
                with open(os.path.join(directory, "%s_reg%d.dat" % (r["fileprefix"], rid)), "wb") as fh:
                    fh.write(np.uint64(r["writefreq"]).tobytes())
        self._engine = engine

    def ramp(self, simstep: int):
        """the target temperature adjustment of CalcGlobalValues (TemperatureControl.cpp:266-277), before the betas of `simstep`"""
        if not self._measures(simstep):
            return
        for k, r in enumerate(self._regions):
            m = r["ramp"]
            if m and m["update_start"] < simstep <= m["update_stop"]:
                if m["elapsed"] == 0:
                    r["temperature"] = m["start"]
                elif m["update_stop"] == simstep:
                    r["temperature"] = m["end"]
                elif m["elapsed"] % m["update_freq"] == 0:
                    r["temperature"] = m["start"] + m["elapsed"] * m["slope"]
                m["elapsed"] += 1
                self._engine.tempcontrol_target(k + 1, r["temperature"])

    def DoLoopsOverMolecules(self, simstep: int, directory: str | None = None):
        self.ramp(simstep)
        self._engine.temperature_control(simstep)
        if directory is not None:
            self.write(simstep, directory)

    def write(self, simstep: int, directory: str = "."):
        """WriteBetaLogfile (TemperatureControl.cpp:455-488) of every region: on a measuring step with simstep % writefreq == 0 two
        doubles are appended — the sums over slabs AND configurations of betaTrans / betaRot divided by the number of configurations
        (not by the slabs: the reference's quirk, kept) — and the accumulators start again."""
        if not self._measures(simstep):
            return []
        paths = []
        for k, r in enumerate(self._regions):
            if simstep % r["writefreq"] != 0:
                continue
            t = self._engine.tempcontrol_read(k + 1, reset=True)
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = np.float64(1.0) / np.float64(t["configs"])
                rec = np.array([t["beta_trans_sum"] * inv, t["beta_rot_sum"] * inv], dtype="<f8")
            paths.append(os.path.join(directory, "%s_reg%d.dat" % (r["fileprefix"], k + 1)))
            with open(paths[-1], "ab") as fh:
                fh.write(rec.tobytes())
        return paths


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


class Widom:
    """Residual chemical potential from test insertions on the device (ls1hip_widom_*): per slab of the y axis
    mu_res = -T ln(sum_w / n), sum_w the accumulated exp(-dU / T) of the n tests that fell into the slab.

    Multi-rank: every rank samples its own box; the per-rank sum_w and n are ADDITIVE — sum them over the ranks (and over
    runs) and pass the sums to mu_res / render.  Orientations of rotating components are uniformly distributed, unlike the
    reference's fixed reservoir orientation."""

    def __init__(self, engine, component: int, instances: int, T: float, seed: int, slabs: int = 1, cv_min=None, cv_max=None,
                 length_y: float | None = None):
        self.engine, self.T, self.slabs = engine, float(T), int(slabs)
        self.length_y = float(engine.global_len[1] if length_y is None else length_y)
        engine.widom_config(component, instances, T, seed, slabs, cv_min, cv_max)

    def sample(self):
        self.engine.widom_sample()

    @staticmethod
    def mu_res_of(sum_w, n, T):
        """(total, per slab) of -T ln(sum_w / n); nan where n = 0, +inf where every test overlapped."""
        sum_w, n = np.asarray(sum_w, dtype=np.float64), np.asarray(n, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            per = np.where(n > 0, -T * np.log(sum_w / n), np.nan)
            tot = -T * np.log(sum_w.sum() / n.sum()) if n.sum() > 0 else float("nan")
        return float(tot), per

    def mu_res(self):
        t = self.engine.widom_read()
        return self.mu_res_of(t["sum_w"], t["n"], self.T)

    @staticmethod
    def render(sum_w, n, T, length_y):
        """The table of write(): `# slab y_mid n <w> mu_res`, one line per slab, then `# total n <w> mu_res`."""
        sum_w, n = np.asarray(sum_w, dtype=np.float64), np.asarray(n, dtype=np.uint64)
        tot, per = Widom.mu_res_of(sum_w, n, T)
        out = ["# slab\ty_mid\tn\t<w>\tmu_res\n"]
        for k in range(len(n)):
            w = sum_w[k] / float(n[k]) if n[k] else float("nan")
            out.append("%d\t%.10g\t%d\t%.12e\t%.12e\n" % (k, (k + 0.5) * length_y / len(n), int(n[k]), w, per[k]))
        nt = int(n.sum())
        out.append("# total\t%d\t%.12e\t%.12e\n" % (nt, sum_w.sum() / nt if nt else float("nan"), tot))
        return "".join(out)

    def write(self, path):
        t = self.engine.widom_read()
        with open(path, "w") as fh:
            fh.write(self.render(t["sum_w"], t["n"], self.T, self.length_y))


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
        if isinstance(cellProcessor, ODFCellProcessor):
            # the ODF traversal: one sampling pass over the same cells (arrays stay on the device until ODF::collect)
            cellProcessor._odf._configure(self.engine)
            self.engine.odf_sample()
            return
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
