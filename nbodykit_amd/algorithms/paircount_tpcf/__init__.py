from .tpcf import SimulationBox2PCF
from .estimators import WedgeBinnedStatistic
