from .simbox import SimulationBoxPairCount
