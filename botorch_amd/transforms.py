"""Input transforms (botorch/models/transforms/input.py): Normalize, the learned
Kumaraswamy Warp and their chain.

Every transform here is a per-column map ``v = (x - offset) / range`` followed,
on flagged columns, by ``z = 1 - (1 - u^a)^b`` with ``u = clamp(v (1 - 2 eps) +
eps, eps, 1 - eps)``, so one pass of ``bo_input_warp`` (csrc/warp.hip, reached
through ``torch.ops.bo.input_warp`` with its registered backward) serves
Normalize, Warp and the chain Normalize -> Warp alike.  CPU tensors and d > 64
take ``warp_torch``, the same formulas in torch.  Both evaluate the Kumaraswamy
step in log space: t = a log u, s = log(-expm1(t)), z = -expm1(b s).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional

import torch
from torch import Tensor, nn

from .exceptions import UnsupportedError
from .models import _TrackedModule

CONCENTRATION_LOWER = 1e-4  # Warp._min_concentration_level


def warp_torch(X: Tensor, offset: Tensor, rscale: Tensor, conc1: Tensor, conc0: Tensor,
               mask: int, eps: float) -> Tensor:
    """bo_input_warp's contract in torch (differentiable in X, conc1, conc0)."""
    d = X.shape[-1]
    v = (X - offset) * rscale
    if not mask:
        return v
    u = (v * (1.0 - 2.0 * eps) + eps).clamp(eps, 1.0 - eps)
    s = torch.log(-torch.expm1(conc1 * torch.log(u)))
    z = -torch.expm1(conc0 * s)
    flag = torch.tensor([(mask >> c) & 1 for c in range(d)], dtype=torch.bool, device=X.device)
    return torch.where(flag, z, v)


def apply_columns(X: Tensor, offset, rscale, conc1, conc0, mask: int, eps: float) -> Tensor:
    """The column map on X (... x d): the HIP kernel for device tensors up to
    d = 64, warp_torch otherwise."""
    from . import kernels
    if X.is_cuda and X.shape[-1] <= kernels.WARP_MAX_DIM and X.dtype == torch.float64:
        from . import ops  # noqa: F401  (registers torch.ops.bo)
        # the op's schema takes a signed 64-bit int: bit 63 (column 63) rides as the sign
        signed = mask - (1 << 64) if mask >= (1 << 63) else mask
        return torch.ops.bo.input_warp(X, offset, rscale, conc1, conc0, signed, eps)
    return warp_torch(X, offset, rscale, conc1, conc0, mask, eps)


class InputTransform(_TrackedModule):
    """models/transforms/input.py:37-155."""

    transform_on_train = True
    transform_on_eval = True
    transform_on_fantasize = True
    is_one_to_many = False
    _eps = 1e-7

    def _flags(self, transform_on_train, transform_on_eval, transform_on_fantasize, reverse,
               batch_shape):
        if reverse:
            raise UnsupportedError(f"{type(self).__name__}: reverse=True is not on the "
                                   "accelerated path")
        if batch_shape is not None and tuple(batch_shape) != ():
            raise UnsupportedError(f"{type(self).__name__}: batch_shape other than () is not on "
                                   "the accelerated path")
        self.transform_on_train = transform_on_train
        self.transform_on_eval = transform_on_eval
        self.transform_on_fantasize = transform_on_fantasize
        self.reverse = False
        self.batch_shape = torch.Size()

    def columns(self, d: int):
        """(offset, rscale, conc1, conc0, mask) of this transform as d-vectors."""
        raise NotImplementedError

    def _applies(self) -> bool:
        return self.transform_on_train if self.training else self.transform_on_eval

    def transform(self, X: Tensor) -> Tensor:
        return apply_columns(X, *self.columns(X.shape[-1]), self._eps)

    def untransform(self, X: Tensor) -> Tensor:
        raise NotImplementedError

    def forward(self, X: Tensor) -> Tensor:
        return self.transform(X) if self._applies() else X

    def preprocess_transform(self, X: Tensor) -> Tensor:
        return self.transform(X) if self.transform_on_train else X

    def state_key(self) -> tuple:
        """Identity and version of every parameter and buffer: changes with any of them."""
        return tuple((t.data_ptr(), t._version)
                     for t in list(self.parameters()) + list(self.buffers()))

    def eval_columns(self, d: int):
        """``columns(d)`` detached, built once per state of the transform (the acquisition
        calls' route: the gradient goes to X, not to the transform's parameters)."""
        key = (d, self.state_key())
        hit = self.__dict__.get("_eval_columns")
        if hit is None or hit[0] != key:
            cols = self.columns(d)
            hit = (key, tuple(c.detach() for c in cols[:4]) + (cols[4],))
            self.__dict__["_eval_columns"] = hit
        return hit[1]

    def eval_transform(self, X: Tensor) -> Tensor:
        """The eval-mode forward whatever the module's mode (no bounds are learned),
        differentiable in X only."""
        return apply_columns(X, *self.eval_columns(X.shape[-1]), self._eps) \
            if self.transform_on_eval else X


class Normalize(InputTransform):
    """Min-max scaling to the unit cube (input.py:490-640).  Without ``bounds`` the
    bounds are learned from the inputs seen in train mode."""

    def __init__(self, d: int, indices: Optional[List[int]] = None, bounds: Optional[Tensor] = None,
                 batch_shape=(), transform_on_train: bool = True, transform_on_eval: bool = True,
                 transform_on_fantasize: bool = True, reverse: bool = False,
                 min_range: float = 1e-8, learn_bounds: Optional[bool] = None,
                 almost_zero: float = 1e-12):
        super().__init__()
        self._flags(transform_on_train, transform_on_eval, transform_on_fantasize, reverse,
                    batch_shape)
        self._d = d
        idx = list(range(d)) if indices is None else [int(i) for i in indices]
        if not idx or len(set(idx)) != len(idx) or min(idx) < 0 or max(idx) >= d:
            raise ValueError(f"Normalize: indices {idx} for d = {d}")
        self.register_buffer("indices", torch.tensor(idx, dtype=torch.long))
        self.learn_coefficients = (bounds is None) if learn_bounds is None else bool(learn_bounds)
        self.min_range, self.almost_zero = float(min_range), float(almost_zero)
        if bounds is not None:
            bounds = torch.as_tensor(bounds, dtype=torch.float64)
            if bounds.dim() != 2:
                raise UnsupportedError("Normalize: batched bounds are not on the accelerated path")
            if indices is not None and bounds.shape[-1] == d:
                bounds = bounds[:, idx]
            if bounds.shape[-1] != len(idx):
                raise ValueError("Dimensions of provided `bounds` are incompatible with "
                                 f"transform_dimension = {len(idx)}!")
            offset, coefficient = bounds[0:1], bounds[1:2] - bounds[0:1]
        else:
            offset = torch.zeros(1, len(idx), dtype=torch.float64)
            coefficient = torch.ones(1, len(idx), dtype=torch.float64)
        self.register_buffer("_offset", offset.clone())
        self.register_buffer("_coefficient", coefficient.clone())

    @property
    def offset(self) -> Tensor:
        return self._offset

    @property
    def coefficient(self) -> Tensor:
        return self._coefficient

    mins, ranges = offset, coefficient

    @property
    def bounds(self) -> Tensor:
        return torch.cat([self._offset, self._offset + self._coefficient], dim=-2)

    @property
    def learn_bounds(self) -> bool:
        return self.learn_coefficients

    def _update_coefficients(self, X: Tensor) -> None:
        """input.py:611-622."""
        Xi = X.detach().reshape(-1, X.shape[-1]).to(torch.float64)[:, self.indices.to(X.device)]
        offset = Xi.amin(dim=0, keepdim=True)
        coefficient = Xi.amax(dim=0, keepdim=True) - offset
        small = coefficient < self.min_range
        coefficient = torch.where(small, torch.ones_like(coefficient), coefficient)
        offset = torch.where(small, torch.zeros_like(offset), offset)
        if self._offset.device == offset.device and self._offset.shape == offset.shape:
            # in place, and only on a change: the buffers' identity and version are part of
            # the model's cache key
            if not (torch.equal(self._offset, offset)
                    and torch.equal(self._coefficient, coefficient)):
                self._offset.copy_(offset)
                self._coefficient.copy_(coefficient)
        else:
            self._coefficient, self._offset = coefficient, offset

    def columns(self, d: int):
        if d != self._d:
            raise ValueError(f"Wrong input dimension. Received {d}, expected {self._d}.")
        dev = self._offset.device
        idx = self.indices
        offset = torch.zeros(d, dtype=torch.float64, device=dev).index_copy(0, idx, self._offset[0])
        rscale = torch.ones(d, dtype=torch.float64, device=dev).index_copy(
            0, idx, 1.0 / self._coefficient[0])
        one = torch.ones(d, dtype=torch.float64, device=dev)
        return offset, rscale, one, one, 0

    def transform(self, X: Tensor) -> Tensor:
        if self.learn_coefficients and self.training:
            if X.shape[-1] != self._d:
                raise ValueError(f"Wrong input dimension. Received {X.shape[-1]}, "
                                 f"expected {self._d}.")
            self._update_coefficients(X)
        return super().transform(X)

    def untransform(self, X: Tensor) -> Tensor:
        offset, rscale, _, _, _ = self.columns(X.shape[-1])
        return X / rscale + offset


class Warp(InputTransform):
    """Learned Kumaraswamy input warping (input.py:922-1060): column i of ``indices`` maps
    to 1 - (1 - u^a_i)^b_i, a = concentration1, b = concentration0, both bounded below by
    1e-4 and fitted with the GP's hyperparameters."""

    _min_concentration_level = CONCENTRATION_LOWER

    def __init__(self, indices: List[int], transform_on_train: bool = True,
                 transform_on_eval: bool = True, transform_on_fantasize: bool = True,
                 reverse: bool = False, eps: float = 1e-7, concentration1_prior=None,
                 concentration0_prior=None, batch_shape=None):
        super().__init__()
        self._flags(transform_on_train, transform_on_eval, transform_on_fantasize, reverse,
                    batch_shape)
        idx = [int(i) for i in indices]
        if not idx or len(set(idx)) != len(idx) or min(idx) < 0:
            raise ValueError(f"Warp: indices {idx}")
        self.register_buffer("indices", torch.tensor(idx, dtype=torch.long))
        self._eps = float(eps)
        self.concentration1_prior = concentration1_prior
        self.concentration0_prior = concentration0_prior
        for name in ("concentration1", "concentration0"):
            setattr(self, "raw_" + name, nn.Parameter(torch.ones(len(idx), dtype=torch.float64)))

    @property
    def concentration1(self) -> Tensor:
        return self.raw_concentration1

    @property
    def concentration0(self) -> Tensor:
        return self.raw_concentration0

    def _set(self, name: str, value) -> None:
        p = getattr(self, name)
        with torch.no_grad():
            p.copy_(torch.as_tensor(value, dtype=torch.float64).to(p.device).expand_as(p))

    @concentration1.setter
    def concentration1(self, value):
        self._set("raw_concentration1", value)

    @concentration0.setter
    def concentration0(self, value):
        self._set("raw_concentration0", value)

    def mask(self, d: int) -> int:
        idx = self.indices.tolist()
        if max(idx) >= d:
            raise ValueError(f"Warp: indices {idx} for d = {d}")
        return sum(1 << i for i in idx)

    def columns(self, d: int):
        dev = self.raw_concentration1.device
        one = torch.ones(d, dtype=torch.float64, device=dev)
        conc1 = one.index_copy(0, self.indices, self.raw_concentration1)
        conc0 = one.index_copy(0, self.indices, self.raw_concentration0)
        return torch.zeros_like(one), one, conc1, conc0, self.mask(d)

    def untransform(self, X: Tensor) -> Tensor:
        """The inverse CDF, then the inverse of the eps shrinkage."""
        _, _, a, b, mask = self.columns(X.shape[-1])
        u = torch.exp(torch.log(-torch.expm1(torch.log1p(-X.clamp(0.0, 1.0)) / b)) / a)
        x = (u - self._eps) / (1.0 - 2.0 * self._eps)
        flag = torch.tensor([(mask >> c) & 1 for c in range(X.shape[-1])], dtype=torch.bool,
                            device=X.device)
        return torch.where(flag, x, X)


class InputPerturbation(InputTransform):
    """Each input with a fixed set of perturbations added (or multiplied in)
    (input.py:1316-1441): ``batch x q x d`` becomes ``batch x (q n_w) x d``, the n_w
    perturbed copies of input i in rows ``i n_w .. (i + 1) n_w``, clamped to ``bounds``
    when given.  With a risk measure (``risk_measures``) as the MC objective this is
    risk-averse optimisation under input noise.  ``perturbation_set``: an n_w x d' tensor,
    d' = len(indices) or d; a callable set (input-dependent perturbations) is not on the
    accelerated path.  It applies at prediction only: the training inputs stay as they are."""

    is_one_to_many = True
    transform_on_fantasize = False

    def __init__(self, perturbation_set: Tensor, bounds: Optional[Tensor] = None,
                 indices: Optional[List[int]] = None, multiplicative: bool = False,
                 transform_on_train: bool = False, transform_on_eval: bool = True):
        super().__init__()
        if not isinstance(perturbation_set, Tensor):
            raise UnsupportedError("InputPerturbation: a callable perturbation_set is not on the "
                                   "accelerated path (pass an n_w x d tensor)")
        if perturbation_set.dim() != 2:
            raise ValueError("`perturbation_set` must be an `n_p x d`-dim tensor!")
        self.register_buffer("perturbation_set", perturbation_set.to(torch.float64))
        if bounds is not None:
            if bounds.shape[-1] != perturbation_set.shape[-1]:
                raise ValueError("`bounds` must have the same number of columns (last dimension) "
                                 f"as the `perturbation_set`! Got {bounds.shape[-1]} and "
                                 f"{perturbation_set.shape[-1]}.")
            self.register_buffer("bounds", bounds.to(torch.float64))
        else:
            self.bounds = None
        self.indices = None if indices is None else [int(i) for i in indices]
        if self.indices is not None and len(self.indices) != perturbation_set.shape[-1]:
            raise ValueError(f"InputPerturbation: {len(self.indices)} indices for a "
                             f"perturbation_set of {perturbation_set.shape[-1]} columns")
        self.multiplicative = bool(multiplicative)
        self.transform_on_train = bool(transform_on_train)
        self.transform_on_eval = bool(transform_on_eval)
        self.reverse = False
        self.batch_shape = torch.Size()

    @property
    def n_w(self) -> int:
        return self.perturbation_set.shape[0]

    def columns(self, d: int):
        raise UnsupportedError("InputPerturbation is no per-column map")

    def transform(self, X: Tensor) -> Tensor:
        p = self.perturbation_set.to(X)
        n_w, q, d = p.shape[0], X.shape[-2], X.shape[-1]
        if (p.shape[1] if self.indices is None else max(self.indices) + 1) > d or (
                self.indices is None and p.shape[1] != d):
            raise ValueError(f"Wrong input dimension. Received {d}, the perturbation_set has "
                             f"{p.shape[1]} columns.")
        Xe = X.unsqueeze(-2).expand(*X.shape[:-1], n_w, d)  # ... x q x n_w x d
        sub = Xe if self.indices is None else Xe[..., self.indices]
        sub = sub * p if self.multiplicative else sub + p
        if self.bounds is not None:
            b = self.bounds.to(X)
            sub = torch.maximum(torch.minimum(sub, b[1]), b[0])
        if self.indices is None:
            Y = sub
        else:
            idx = torch.tensor(self.indices, device=X.device)
            Y = Xe.index_copy(-1, idx, sub)
        return Y.reshape(*X.shape[:-2], q * n_w, d)

    def eval_transform(self, X: Tensor) -> Tensor:
        return self.transform(X) if self.transform_on_eval else X

    def untransform(self, X: Tensor) -> Tensor:
        raise UnsupportedError("InputPerturbation: a one-to-many transform has no inverse")


class ChainedInputTransform(InputTransform):
    """input.py:158-260: the members applied in order.  Normalize followed directly by
    Warp runs as one pass of the kernel."""

    def __init__(self, **transforms: InputTransform):
        super().__init__()
        self._names = list(transforms)
        for name, tf in transforms.items():
            if isinstance(tf, InputPerturbation):
                raise UnsupportedError(f"ChainedInputTransform: member {name!r} is an "
                                       "InputPerturbation, which is on the accelerated path "
                                       "only as a model's sole input transform")
            if not isinstance(tf, InputTransform) or isinstance(tf, ChainedInputTransform):
                raise UnsupportedError(f"ChainedInputTransform: member {name!r} is not a "
                                       "Normalize or Warp of this library")
            self.add_module(name, tf)
        self.transform_on_train = any(tf.transform_on_train for tf in self.values())
        self.transform_on_eval = any(tf.transform_on_eval for tf in self.values())
        self.transform_on_fantasize = any(tf.transform_on_fantasize for tf in self.values())

    def keys(self):
        return list(self._names)

    def values(self):
        return [self._modules[k] for k in self._names]

    def items(self):
        return OrderedDict((k, self._modules[k]) for k in self._names).items()

    def __getitem__(self, name: str) -> InputTransform:
        return self._modules[name]

    def _run(self, X: Tensor, members: list, learn: bool = True) -> Tensor:
        i = 0
        while i < len(members):
            tf = members[i]
            nxt = members[i + 1] if i + 1 < len(members) else None
            if isinstance(tf, Normalize) and isinstance(nxt, Warp):
                if learn and tf.learn_coefficients and tf.training:
                    tf._update_coefficients(X)
                cols = (lambda t: t.columns(X.shape[-1])) if learn else (
                    lambda t: t.eval_columns(X.shape[-1]))
                offset, rscale, _, _, _ = cols(tf)
                _, _, conc1, conc0, mask = cols(nxt)
                X = apply_columns(X, offset, rscale, conc1, conc0, mask, nxt._eps)
                i += 2
            else:
                X = tf.transform(X) if learn else tf.eval_transform(X)
                i += 1
        return X

    def transform(self, X: Tensor) -> Tensor:
        return self._run(X, self.values())

    def forward(self, X: Tensor) -> Tensor:
        return self._run(X, [tf for tf in self.values() if tf._applies()])

    def preprocess_transform(self, X: Tensor) -> Tensor:
        return self._run(X, [tf for tf in self.values() if tf.transform_on_train])

    def eval_transform(self, X: Tensor) -> Tensor:
        return self._run(X, [tf for tf in self.values() if tf.transform_on_eval], learn=False)

    def untransform(self, X: Tensor) -> Tensor:
        for tf in reversed(self.values()):
            X = tf.untransform(X)
        return X


def split_chain(tf: InputTransform):
    """(normalize or None, warp or None) of an admitted transform: Normalize, Warp, or the
    chain Normalize -> Warp; anything else raises UnsupportedError."""
    members = tf.values() if isinstance(tf, ChainedInputTransform) else [tf]
    kinds = [type(m) for m in members]
    if kinds == [Normalize]:
        return members[0], None
    if kinds == [Warp]:
        return None, members[0]
    if kinds == [Normalize, Warp]:
        return members[0], members[1]
    raise UnsupportedError(
        "input_transform: Normalize, Warp, or ChainedInputTransform(Normalize, Warp) in that "
        f"order are on the accelerated path, got {[k.__name__ for k in kinds]}")


__all__ = ["InputTransform", "Normalize", "Warp", "ChainedInputTransform", "InputPerturbation",
           "warp_torch"]
