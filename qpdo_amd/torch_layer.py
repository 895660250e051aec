"""Training through a resident fleet: a torch.autograd.Function over solver.Fleet's device calls.

    fleet = solver.Fleet(probs, matrix_updates=True, adjoint=True)
    layer = FleetQP(fleet)
    x, y = layer(q, l, u, Q_values, A_values)       # packed GPU tensors (Fleet.packed_layout / packed_matrix_layout)
    loss(x, y).backward()                           # q.grad, l.grad, u.grad, Q_values.grad, A_values.grad

Forward is the fleet's control step  update_matrices_device -> update_device -> warm_start_last_device -> solve_device  on torch's current
stream; backward is ONE adjoint_device call on the current stream (qpdo_amd_fleet_adjoint_dev, include/qpdo_amd_ext.h).  Nothing waits for the
host.  The fleet holds ONE solution: a backward belongs to the most recent forward, and one that comes after the fleet has moved on raises."""
import torch

ON_FAILURE = ("nan", "zero")


class _FleetQPFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, q, l, u, Q_values, A_values):
        fleet = layer.fleet
        if Q_values is not None or A_values is not None:
            fleet.update_matrices_device(Q_values=None if Q_values is None else Q_values.detach(), A_values=None if A_values is None else A_values.detach())
        if q is not None or l is not None or u is not None:
            fleet.update_device(q=None if q is None else q.detach(), l=None if l is None else l.detach(), u=None if u is None else u.detach())
        if layer.warm_start_last:
            fleet.warm_start_last_device()
        out = fleet.solve_device()
        layer.status = out["status"].clone()
        ctx.layer, ctx.serial = layer, fleet.solve_serial
        x, y = out["x"].clone(), out["y"].clone()
        return x, y

    @staticmethod
    def backward(ctx, gx, gy):
        layer, fleet = ctx.layer, ctx.layer.fleet
        if fleet.solve_serial != ctx.serial:
            raise RuntimeError("FleetQP.backward: the fleet has been solved again since this forward (solve %d, now %d); a fleet holds one "
                               "solution -- call backward before the next forward" % (ctx.serial, fleet.solve_serial))
        need = ctx.needs_input_grad[1:]                      # q, l, u, Q_values, A_values
        matrices = bool(need[3] or need[4])
        gx = torch.zeros_like(fleet._dev_out["x"]) if gx is None else gx.contiguous()
        out = fleet.adjoint_device(gx, None if gy is None else gy.contiguous(), matrices=matrices)
        layer.adjoint_status = out["status"].clone()
        grads = []
        for want, key in zip(need, ("dq", "dl", "du", "dQ_values", "dA_values")):
            if not want:
                grads.append(None)
                continue
            g = out[key].clone()
            if layer.on_failure == "zero":
                g = _zero_failed(layer, key, g)
            grads.append(g)
        return (None, *grads)


def _zero_failed(layer, key, g):
    """the slices of items with code != 0 replaced by zeros, on the device (no host wait): a mask per element from the item's code"""
    code = layer.adjoint_status[:, 0]
    idx = layer._item_of[key]
    if idx.numel() == 0:
        return g
    return torch.where(code[idx] != 0, torch.zeros_like(g), g)


class FleetQP(torch.nn.Module):
    """x, y = layer(q, l, u, Q_values=None, A_values=None): the fleet's solutions as differentiable functions of its packed inputs.
    fleet: a solver.Fleet created with adjoint=True (and matrix_updates=True if Q_values / A_values are to be passed).  None inputs are left
    as they are in the fleet.  warm_start_last: start every solve from the previous solution.  on_failure: what the gradient slices of an item
    whose adjoint was not delivered (status code != 0: not solved, not accepted) hold -- "nan" (as the call returns them) or "zero".
    layer.status: (count, 3) int64 of the last forward (status_val, iterations, oterations); layer.adjoint_status: (count, 3) int64 of the last
    backward (code, sweeps, active rows)."""

    def __init__(self, fleet, warm_start_last=True, on_failure="nan"):
        super().__init__()
        if on_failure not in ON_FAILURE:
            raise ValueError("on_failure: expected one of %r, got %r" % (ON_FAILURE, on_failure))
        self.fleet, self.warm_start_last, self.on_failure = fleet, bool(warm_start_last), on_failure
        self.status, self.adjoint_status = None, None
        self._item_of = None

    def _build_item_index(self):
        """per output array, the item every element belongs to (GPU int64 tensors; built once from the packed layouts)"""
        import numpy as np
        f = self.fleet
        no, mo = f.packed_layout()
        dev = torch.device("cuda", f._device)

        def owner(off):
            return torch.from_numpy(np.repeat(np.arange(f.count), np.diff(off))).to(dev)
        idx = dict(dq=owner(no), dl=owner(mo), du=owner(mo))
        try:
            qo, ao = f.packed_matrix_layout()
            idx.update(dQ_values=owner(qo), dA_values=owner(ao))
        except RuntimeError:
            pass
        self._item_of = idx

    def forward(self, q=None, l=None, u=None, Q_values=None, A_values=None):
        if self.on_failure == "zero" and self._item_of is None:
            self._build_item_index()
        return _FleetQPFunction.apply(self, q, l, u, Q_values, A_values)
