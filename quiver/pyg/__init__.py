from .sage_sampler import (GraphSageSampler, MixedGraphSageSampler, SampleJob,
                           Adj, LinkBatch, TemporalBatch,
                           SubgraphBatch)

__all__ = ["GraphSageSampler", "MixedGraphSageSampler", "SampleJob", "Adj",
           "LinkBatch", "TemporalBatch", "SubgraphBatch"]
