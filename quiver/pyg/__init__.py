from .sage_sampler import (GraphSageSampler, MixedGraphSageSampler, SampleJob,
                           Adj, LinkBatch)

__all__ = ["GraphSageSampler", "MixedGraphSageSampler", "SampleJob", "Adj",
           "LinkBatch"]
