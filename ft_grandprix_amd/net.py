"""Network drivers: a trained MLP as a device policy (include/ftgp.h "Network drivers").

A ``NetSpec`` is everything ``ftgp_set_net`` / ``ftgp_set_net_frame`` / ``ftgp_set_net_rivals`` take: which beams of the scan the network
reads, whether the five state inputs follow, whether the track-frame row (``frame``, ``lookahead``, ``lookahead_stride``) follows those
and the rival row (``rivals``, ``n_rivals``) follows that, the layers in torch's ``nn.Linear`` layout, the two activations and the output map.  ``from_torch`` freezes an ``nn.Sequential`` of
``Linear`` / ``ReLU`` / ``Tanh`` / ``Identity`` into one; ``save`` / ``load`` keep it as an ``.npz``.

The library evaluates the network in binary32 with a fixed order of operations and its own TANH (a continued fraction, within 2.7e-7
of ``tanh``): a network trained with torch's ``tanh`` runs with activations that differ in the seventh digit.
"""
from dataclasses import dataclass, field

import numpy as np

from . import capi


@dataclass
class NetSpec:
    layers: list                      # [(W float32 [n_out, n_in], b float32 [n_out]), ...]
    pool: int
    max_range: float
    beam_first: int
    n_beams: int
    use_state: bool = False
    hidden_act: str = "tanh"
    out_act: str = "tanh"
    out_scale: tuple = (1.0, 1.0)
    out_offset: tuple = (0.0, 0.0)
    frame: bool = False               # the track-frame row behind the beams and the state inputs (ftgp_set_net_frame)
    lookahead: int = 0                # look-ahead points of that row; > 0 turns ``frame`` on, as in DeviceVecEnv
    lookahead_stride: int = 1         # path points between two of them
    rivals: bool = False              # the rival row of the car's env behind all of those (ftgp_set_net_rivals)
    n_rivals: int = 0                 # mate slots of that row, 0 .. 7; > 0 turns ``rivals`` on, as in DeviceVecEnv
    _flat: np.ndarray = field(default=None, repr=False, compare=False)

    def __post_init__(self):
        self.layers = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)) for W, b in self.layers]
        self.out_scale = tuple(float(x) for x in self.out_scale)
        self.out_offset = tuple(float(x) for x in self.out_offset)
        f = capi.net_frame(self.frame, self.lookahead, self.lookahead_stride)      # the ranges, before anything is loaded
        self.frame, self.lookahead, self.lookahead_stride = bool(f.enabled), int(f.n_ahead), int(f.stride)
        r = capi.net_rivals(self.rivals, self.n_rivals)
        self.rivals, self.n_rivals = bool(r.enabled), int(r.n_rivals)
        _, self._flat = capi.net_desc(self.layers, **self.input_fields())      # every check that needs no handle

    def input_fields(self) -> dict:
        return dict(pool=self.pool, max_range=self.max_range, beam_first=self.beam_first, n_beams=self.n_beams, use_state=self.use_state,
                    hidden_act=self.hidden_act, out_act=self.out_act, out_scale=self.out_scale, out_offset=self.out_offset,
                    frame=self.frame, lookahead=self.lookahead, lookahead_stride=self.lookahead_stride, rivals=self.rivals, n_rivals=self.n_rivals)

    @property
    def n_frame(self) -> int:
        """Frame entries at the end of the input vector: 0 without frame inputs."""
        return capi.FRAME_FIXED + 2 * self.lookahead if self.frame else 0

    @property
    def n_rival(self) -> int:
        """Rival entries at the end of the input vector, behind the frame entries: 0 without rival inputs."""
        return capi.RIVAL_FIXED + capi.RIVAL_FLOATS * self.n_rivals if self.rivals else 0

    @property
    def n_in(self) -> int:
        return self.n_beams + (capi.NET_STATE_INPUTS if self.use_state else 0) + self.n_frame + self.n_rival

    @property
    def widths(self) -> tuple:
        """(n_in, outputs of layer 0, ...): two specs of equal shape can replace one another through ftgp_set_net_device."""
        return (self.n_in,) + tuple(W.shape[0] for W, _ in self.layers)

    def shape_key(self) -> tuple:
        d = self.input_fields()
        return (self.widths,) + tuple(d[k] for k in sorted(d))

    def flat_params(self) -> np.ndarray:
        """float32, ftgp_set_net's layout: per layer W[n_out][n_in], then b[n_out]."""
        return self._flat.copy()

    @property
    def param_count(self) -> int:
        """Floats of ``flat_params``: the row width of a population (``stack_params``, ftgp_set_net_population)."""
        return int(self._flat.size)

    def with_params(self, flat) -> "NetSpec":
        """A spec of the same shape and input fields with the parameters of one flat float32 row in ``flat_params``' layout -- a
        member of a population, the winner for example."""
        flat = np.asarray(flat.detach().cpu().numpy() if hasattr(flat, "detach") else flat)
        if flat.dtype != np.float32 or flat.shape != (self.param_count,):
            raise ValueError(f"flat: float32 [{self.param_count}], got {flat.dtype} {flat.shape}")
        layers, o = [], 0
        for W, b in self.layers:
            layers.append((flat[o:o + W.size].reshape(W.shape), flat[o + W.size:o + W.size + b.size]))
            o += W.size + b.size
        return NetSpec(layers, **self.input_fields())

    def check_window(self, n_rays: int):
        capi.check_net_window(n_rays, self.pool, self.beam_first, self.n_beams)

    def save(self, path):
        arrays = {}
        for l, (W, b) in enumerate(self.layers):
            arrays[f"W{l}"], arrays[f"b{l}"] = W, b
        np.savez(path, n_layers=len(self.layers), pool=self.pool, max_range=np.float32(self.max_range), beam_first=self.beam_first,
                 n_beams=self.n_beams, use_state=int(self.use_state), hidden_act=self.hidden_act, out_act=self.out_act,
                 out_scale=np.asarray(self.out_scale, dtype=np.float32), out_offset=np.asarray(self.out_offset, dtype=np.float32),
                 frame=int(self.frame), lookahead=self.lookahead, lookahead_stride=self.lookahead_stride,
                 rivals=int(self.rivals), n_rivals=self.n_rivals, **arrays)


def load(path) -> NetSpec:
    with np.load(path, allow_pickle=False) as z:
        layers = [(z[f"W{l}"], z[f"b{l}"]) for l in range(int(z["n_layers"]))]
        # (a file written before the frame inputs existed has none of the three keys: the frame is off)
        frame = dict(frame=bool(int(z["frame"])), lookahead=int(z["lookahead"]), lookahead_stride=int(z["lookahead_stride"])) if "frame" in z.files else {}
        # (... and one written before the rival inputs existed has neither of their two keys: rivals are off)
        if "rivals" in z.files:
            frame.update(rivals=bool(int(z["rivals"])), n_rivals=int(z["n_rivals"]))
        return NetSpec(layers, pool=int(z["pool"]), max_range=float(z["max_range"]), beam_first=int(z["beam_first"]), n_beams=int(z["n_beams"]),
                       use_state=bool(int(z["use_state"])), hidden_act=str(z["hidden_act"]), out_act=str(z["out_act"]),
                       out_scale=tuple(z["out_scale"]), out_offset=tuple(z["out_offset"]), **frame)


def stack_params(specs) -> np.ndarray:
    """float32 [len(specs), param_count]: the flat parameters of specs of one shape, a row per member -- what
    ``set_net_population`` takes.  Specs whose ``shape_key()`` differ are refused (ValueError)."""
    specs = list(specs)
    if not specs or not all(isinstance(s, NetSpec) for s in specs):
        raise ValueError("stack_params: a non-empty list of NetSpec")
    for i, s in enumerate(specs):
        if s.shape_key() != specs[0].shape_key():
            raise ValueError(f"stack_params: spec {i} differs in shape or input fields from spec 0: {s.shape_key()} != {specs[0].shape_key()}")
    return np.stack([s.flat_params() for s in specs])


def _torch_layers(module, who: str):
    """(layers, activation names) of an ``nn.Sequential(Linear, act, ..., Linear[, act])``: the module rules of ``from_torch``."""
    import torch.nn as nn
    if not isinstance(module, nn.Sequential):
        raise TypeError(f"{who} takes an nn.Sequential of Linear / ReLU / Tanh / Identity, got {type(module).__name__}")
    names = {nn.ReLU: "relu", nn.Tanh: "tanh", nn.Identity: "identity"}
    layers, acts = [], []
    for i, m in enumerate(module):
        if isinstance(m, nn.Linear):
            if m.bias is None:
                raise ValueError(f"module {i}: a Linear without bias is not supported (give it a zero bias)")
            layers.append((m.weight.detach().cpu().numpy().astype(np.float32), m.bias.detach().cpu().numpy().astype(np.float32)))
            acts.append("identity")
        elif type(m) in names:
            if not layers or acts[-1] != "identity":
                raise ValueError(f"module {i}: {type(m).__name__} must follow a Linear, one activation per layer")
            acts[-1] = names[type(m)]
        else:
            raise TypeError(f"module {i}: {type(m).__name__} is not supported: Linear, ReLU, Tanh and Identity only")
    if not layers:
        raise ValueError("the module has no Linear layer")
    if len(set(acts[:-1])) > 1:
        raise ValueError(f"every hidden layer must use the same activation, got {acts[:-1]}")
    return layers, acts


@dataclass
class ValueSpec:
    """Everything ``ftgp_set_value_net`` takes: the layers of a critic in torch's ``nn.Linear`` layout -- the first one as wide as the
    input vector of the slot it is set on, the last one with a single output --, the two activations and the output map
    ``v = y * out_scale + out_offset``."""
    layers: list                      # [(W float32 [n_out, n_in], b float32 [n_out]), ...]
    hidden_act: str = "tanh"
    out_act: str = "identity"
    out_scale: float = 1.0
    out_offset: float = 0.0
    _flat: np.ndarray = field(default=None, repr=False, compare=False)

    def __post_init__(self):
        self.layers = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)) for W, b in self.layers]
        self.out_scale, self.out_offset = float(self.out_scale), float(self.out_offset)
        _, self._flat = capi.value_desc(self.layers, **self.fields())         # every check that needs no handle

    def fields(self) -> dict:
        return dict(hidden_act=self.hidden_act, out_act=self.out_act, out_scale=self.out_scale, out_offset=self.out_offset)

    @property
    def n_in(self) -> int:
        return int(self.layers[0][0].shape[1])

    @property
    def widths(self) -> tuple:
        return (self.n_in,) + tuple(W.shape[0] for W, _ in self.layers)

    def flat_params(self) -> np.ndarray:
        """float32, ftgp_set_value_net's layout: per layer W[n_out][n_in], then b[n_out]."""
        return self._flat.copy()

    @property
    def param_count(self) -> int:
        return int(self._flat.size)

    def with_params(self, flat) -> "ValueSpec":
        """A spec of the same shape and fields with the parameters of one flat float32 row in ``flat_params``' layout."""
        flat = np.asarray(flat.detach().cpu().numpy() if hasattr(flat, "detach") else flat)
        if flat.dtype != np.float32 or flat.shape != (self.param_count,):
            raise ValueError(f"flat: float32 [{self.param_count}], got {flat.dtype} {flat.shape}")
        layers, o = [], 0
        for W, b in self.layers:
            layers.append((flat[o:o + W.size].reshape(W.shape), flat[o + W.size:o + W.size + b.size]))
            o += W.size + b.size
        return ValueSpec(layers, **self.fields())

    def save(self, path):
        arrays = {}
        for l, (W, b) in enumerate(self.layers):
            arrays[f"W{l}"], arrays[f"b{l}"] = W, b
        np.savez(path, value_net=1, n_layers=len(self.layers), hidden_act=self.hidden_act, out_act=self.out_act,
                 out_scale=np.float32(self.out_scale), out_offset=np.float32(self.out_offset), **arrays)

    @staticmethod
    def load(path) -> "ValueSpec":
        with np.load(path, allow_pickle=False) as z:
            if "value_net" not in z.files:
                raise ValueError(f"{path}: not a value net's file (ValueSpec.save)")
            layers = [(z[f"W{l}"], z[f"b{l}"]) for l in range(int(z["n_layers"]))]
            return ValueSpec(layers, hidden_act=str(z["hidden_act"]), out_act=str(z["out_act"]), out_scale=float(z["out_scale"]),
                             out_offset=float(z["out_offset"]))


def value_from_torch(module, out_scale=1.0, out_offset=0.0) -> ValueSpec:
    """Freeze a critic ``nn.Sequential(Linear, act, ..., Linear[, act])`` under ``from_torch``'s module rules; the last Linear must have
    one output."""
    layers, acts = _torch_layers(module, "value_from_torch")
    if layers[-1][0].shape[0] != 1:
        raise ValueError(f"the last Linear of a value net has exactly 1 output, got {layers[-1][0].shape[0]}")
    hidden = set(acts[:-1])
    return ValueSpec(layers, hidden_act=hidden.pop() if hidden else "tanh", out_act=acts[-1], out_scale=out_scale, out_offset=out_offset)


def from_torch(module, **input_fields) -> NetSpec:
    """Freeze ``nn.Sequential(Linear, act, Linear, act, ..., Linear[, act])`` with act in ReLU / Tanh / Identity.  Every hidden layer
    must use the same activation; a Linear without one behind it has the identity.  ``input_fields``: pool, max_range, beam_first,
    n_beams and optionally use_state, out_scale, out_offset, frame, lookahead, lookahead_stride, rivals, n_rivals.  Anything else in the module is refused."""
    import torch.nn as nn
    if not isinstance(module, nn.Sequential):
        raise TypeError(f"from_torch takes an nn.Sequential of Linear / ReLU / Tanh / Identity, got {type(module).__name__}")
    for k in ("hidden_act", "out_act"):
        if k in input_fields:
            raise TypeError(f"{k} is read from the module")
    names = {nn.ReLU: "relu", nn.Tanh: "tanh", nn.Identity: "identity"}
    layers, acts = [], []
    for i, m in enumerate(module):
        if isinstance(m, nn.Linear):
            if m.bias is None:
                raise ValueError(f"module {i}: a Linear without bias is not supported (give it a zero bias)")
            layers.append((m.weight.detach().cpu().numpy().astype(np.float32), m.bias.detach().cpu().numpy().astype(np.float32)))
            acts.append("identity")
        elif type(m) in names:
            if not layers or acts[-1] != "identity":
                raise ValueError(f"module {i}: {type(m).__name__} must follow a Linear, one activation per layer")
            acts[-1] = names[type(m)]
        else:
            raise TypeError(f"module {i}: {type(m).__name__} is not supported: Linear, ReLU, Tanh and Identity only")
    if not layers:
        raise ValueError("the module has no Linear layer")
    hidden = set(acts[:-1])
    if len(hidden) > 1:
        raise ValueError(f"every hidden layer must use the same activation, got {acts[:-1]}")
    return NetSpec(layers, hidden_act=hidden.pop() if hidden else "tanh", out_act=acts[-1], **input_fields)
