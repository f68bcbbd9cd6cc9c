from .fftpower import (FFTPower, FFTBase, ProjectedFFTPower,
                       project_to_basis)
from .fftcorr import FFTCorr
from .fftrecon import FFTRecon
from .convpower import ConvolvedFFTPower, FKPCatalog, FKPWeightFromNbar
from .zhist import RedshiftHistogram
from .pair_counters import SimulationBoxPairCount, SurveyDataPairCount
from .paircount_tpcf import SimulationBox2PCF, SurveyData2PCF
from .threeptcf import SimulationBox3PCF, SurveyData3PCF
from .fof import FOF
from .kdtree import KDDensity
from .cgm import CylindricalGroups
from .fibercollisions import FiberCollisions
