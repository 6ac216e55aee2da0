"""Sampling strategies over a discrete candidate set (botorch/generation/sampling.py)."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from .objective import IdentityMCObjective


class SamplingStrategy(nn.Module):
    """generation/sampling.py:35-57: draws ``num_samples`` of the N candidates."""

    def forward(self, X: Tensor, num_samples: int = 1) -> Tensor:
        raise NotImplementedError


class MaxPosteriorSampling(SamplingStrategy):
    """generation/sampling.py:60-155: (discrete) Thompson sampling -- each
    posterior sample over the N candidates picks its maximiser under the
    objective.  Without replacement, sample i takes its best candidate that the
    samples before it have not taken."""

    def __init__(self, model, objective=None, posterior_transform=None, replacement: bool = True):
        super().__init__()
        self.model = model
        self.objective = IdentityMCObjective() if objective is None else objective
        self.posterior_transform = posterior_transform
        self.replacement = replacement

    def forward(self, X: Tensor, num_samples: int = 1, observation_noise: bool = False) -> Tensor:
        """X: ``batch_shape x N x d`` -> ``batch_shape x num_samples x d``."""
        posterior = self.model.posterior(X, observation_noise=observation_noise,
                                         posterior_transform=self.posterior_transform)
        samples = posterior.rsample(sample_shape=torch.Size([num_samples]))
        return self.maximize_samples(X, samples, num_samples)

    def maximize_samples(self, X: Tensor, samples: Tensor, num_samples: int = 1) -> Tensor:
        """samples: ``num_samples x batch_shape x N x m``."""
        obj = self.objective(samples, X=X)  # num_samples x batch_shape x N
        if self.replacement:
            picks = obj.argmax(dim=-1)
        else:
            if obj.dim() > 3:
                raise NotImplementedError(
                    "MaxPosteriorSampling without replacement for more than a single "
                    "batch dimension is not yet implemented.")
            # a sample's first num_samples ranks always hold a candidate not yet taken
            ranked = obj.topk(num_samples, dim=-1).indices
            chosen = []
            for i in range(num_samples):
                taken = torch.zeros_like(ranked[i], dtype=torch.bool)
                for c in chosen:
                    taken |= ranked[i] == c.unsqueeze(-1)
                first = (~taken).to(torch.int8).argmax(dim=-1, keepdim=True)
                chosen.append(ranked[i].gather(-1, first).squeeze(-1))
            picks = torch.stack(chosen, dim=0)
        if picks.dim() > 1:  # num_samples x batch_shape -> batch_shape x num_samples
            picks = picks.movedim(0, -1)
        index = picks.unsqueeze(-1).expand(*picks.shape, X.shape[-1])
        return torch.gather(X.expand(*obj.shape[1:], X.shape[-1]), -2, index)
