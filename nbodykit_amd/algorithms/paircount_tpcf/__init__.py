from .tpcf import SimulationBox2PCF, SurveyData2PCF
from .estimators import WedgeBinnedStatistic
