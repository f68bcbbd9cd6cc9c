from .simbox import SimulationBoxPairCount
from .mocksurvey import SurveyDataPairCount
