from .sage_sampler import (GraphSageSampler, MixedGraphSageSampler, SampleJob,
                           Adj, LinkBatch, TemporalBatch)

__all__ = ["GraphSageSampler", "MixedGraphSageSampler", "SampleJob", "Adj",
           "LinkBatch", "TemporalBatch"]
