"""Closed-form parameter values for the fixtures whose state_dict the oracle's `param_shapes` does not cover (reward_input: a
5-channel first convolution).  The value rule is the one of `oracle.dreamer_oracle.make_params`, restated over an explicit
ordered {name: shape} map: one numpy RandomState per tensor, seeded by the tensor's index in the reference's state_dict order.
The fixture generator (scripts/gen_obs_golden.py) loads these values into the reference; the tests load them into the HIP model;
no weight is ever stored."""
import math
from collections import OrderedDict

import numpy as np
import torch


def make_params(shapes, seed=0, dtype=torch.float32):
    """shapes: ordered {name: shape} (the reference's state_dict order)."""
    out = OrderedDict()
    for i, (name, shape) in enumerate(shapes.items()):
        shape = tuple(int(x) for x in shape)
        rs = np.random.RandomState(seed * 100003 + i)
        if name == 'probe_model.dummy':
            v = np.full(shape, 0.25, dtype=np.float64)
        elif len(shape) == 1:
            v = (1.0 if name.endswith('.weight') else 0.0) + 0.05 * rs.uniform(-1, 1, shape)
        else:
            if len(shape) == 4:
                fan_in, fan_out = shape[1] * shape[2] * shape[3], shape[0] * shape[2] * shape[3]
            else:
                fan_out, fan_in = shape
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            v = rs.uniform(-lim, lim, shape)
        out[name] = torch.tensor(v, dtype=dtype)
    return out


def shapes_of_fixture(g):
    """The ordered {name: shape} map a fixture recorded (`param_names`, `param_shapes` padded with -1)."""
    return OrderedDict((str(n), tuple(int(x) for x in s if x >= 0)) for n, s in zip(g['param_names'], g['param_shapes']))
