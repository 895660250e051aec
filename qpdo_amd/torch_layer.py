"""Training through a resident fleet: a torch.autograd.Function over solver.Fleet's device calls.

    fleet = solver.Fleet(probs, matrix_updates=True, adjoint=True)
    layer = FleetQP(fleet)
    x, y = layer(q, l, u, Q_values, A_values)       # packed GPU tensors (Fleet.packed_layout / packed_matrix_layout)
    loss(x, y).backward()                           # q.grad, l.grad, u.grad, Q_values.grad, A_values.grad

Forward is the fleet's control step  update_matrices_device -> update_device -> warm_start_last_device -> solve_device  on torch's current
stream; backward is ONE adjoint_device call on the current stream (qpdo_amd_fleet_adjoint_dev, include/qpdo_amd_ext.h).  Nothing waits for the
host.  The fleet holds ONE solution: a backward belongs to the most recent forward, and one that comes after the fleet has moved on raises.

One QP of any size the direct solvers take (dense LDL', band LDL') goes through WorkspaceQP, over solver.QPDO's host calls:

    qp = solver.QPDO().setup(Q, q, A, l, u)
    layer = WorkspaceQP(qp)
    x, y = layer(q, l, u, Q_values, A_values)       # tensors on any device; the values in the setup's stored pattern
    loss(x, y).backward()

Forward is  update_matrices -> update_bounds -> update_q -> (warm start from the previous x, y) -> solve,  backward ONE qpdo_amd_adjoint call;
the tensors travel through the host, since that API is a host API."""
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
    backward (code, sweeps, active rows).
    layer.tangent(...) and layer.vjp_many(gx, gy) are the forward sensitivity and R backward products of the most recent forward, from one
    factorization per item; their status tensors are kept as layer.tangent_status and layer.vjp_status."""

    def __init__(self, fleet, warm_start_last=True, on_failure="nan"):
        super().__init__()
        if on_failure not in ON_FAILURE:
            raise ValueError("on_failure: expected one of %r, got %r" % (ON_FAILURE, on_failure))
        self.fleet, self.warm_start_last, self.on_failure = fleet, bool(warm_start_last), on_failure
        self.status, self.adjoint_status, self.tangent_status, self.vjp_status = None, None, None, None
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
        x, y = _FleetQPFunction.apply(self, q, l, u, Q_values, A_values)
        self._serial = self.fleet.solve_serial
        return x, y

    # ---- sensitivities of the most recent forward beside autograd: many right-hand sides per factorization ---------------------------------
    def _guard(self, what):
        """the serial guard of backward: the fleet holds ONE solution, that of the most recent forward of this layer"""
        serial, now = getattr(self, "_serial", None), getattr(self.fleet, "solve_serial", 0)
        if serial is None:
            raise RuntimeError("FleetQP.%s: no forward yet" % what)
        if now != serial:
            raise RuntimeError("FleetQP.%s: the fleet has been solved again since this forward (solve %d, now %d); a fleet holds one "
                               "solution -- call %s before the next forward" % (what, serial, now, what))

    def _failed(self, out, keys):
        """on_failure applied to a sensitivity result: "zero" replaces the slices of right-hand sides with code != 0 by zeros (on the device)"""
        res = {k: (None if v is None else v.clone()) for k, v in out.items()}
        if self.on_failure == "zero":
            if self._item_of is None:
                self._build_item_index()
            code = res["status"][..., 0]
            for k, owner in keys.items():
                if res[k] is not None and self._item_of[owner].numel():
                    res[k] = torch.where(code[..., self._item_of[owner]] != 0, torch.zeros_like(res[k]), res[k])
        return res

    def tangent(self, tq=None, tl=None, tu=None, tQ_values=None, tA_values=None, tol=1e-9, max_sweeps=20):
        """The first-order change (dx, dy) of the most recent forward's x, y for a change of its inputs (Fleet.tangent_device; arrays (L,) or
        (R, L)): a dict with dx, dy, active, status, residual.  Raises when the fleet has been solved again since that forward."""
        self._guard("tangent")
        out = self.fleet.tangent_device(*(None if t is None else t.detach().contiguous() for t in (tq, tl, tu, tQ_values, tA_values)), tol=tol, max_sweeps=max_sweeps)
        self.tangent_status = out["status"].clone()
        return self._failed(out, dict(dx="dq", dy="dl"))

    def vjp_many(self, gx, gy=None, matrices=False, tol=1e-9, max_sweeps=20):
        """R vector-Jacobian products of the most recent forward at once (Fleet.adjoint_many_device; gx (R, N), gy (R, M) or None): a dict with
        dq, dl, du, dQ_values, dA_values (matrices=True), active, status, residual, each gradient with the leading R.  Raises when the fleet
        has been solved again since that forward."""
        self._guard("vjp_many")
        out = self.fleet.adjoint_many_device(gx.detach().contiguous(), None if gy is None else gy.detach().contiguous(), matrices=matrices, tol=tol,
                                             max_sweeps=max_sweeps)
        self.vjp_status = out["status"].clone()
        return self._failed(out, dict(dq="dq", dl="dl", du="du", dQ_values="dQ_values", dA_values="dA_values"))


class _WorkspaceQPFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, q, l, u, Q_values, A_values):
        import numpy as np
        import scipy.sparse as sp
        qp = layer.qp

        def host(t):
            return None if t is None else np.ascontiguousarray(t.detach().cpu().numpy(), np.float64)

        def mat(vals, pat, shape):
            return None if vals is None else sp.csc_matrix((host(vals), pat[1], pat[0]), shape=shape)
        if Q_values is not None or A_values is not None:
            qp.update_matrices(Q=mat(Q_values, qp._Qpat, (qp.n, qp.n)), A=mat(A_values, qp._Apat, (qp.m, qp.n)))
        if l is not None or u is not None:
            qp.update_bounds(host(l), host(u))
        if q is not None:
            qp.update_q(host(q))
        if layer.warm_start_last and layer._last is not None:
            qp.warm_start(*layer._last)
        r = qp.solve()
        layer.serial += 1
        layer.status = r["info"]["status_val"]
        layer._last = (r["x"], r["y"]) if np.isfinite(r["x"]).all() and np.isfinite(r["y"]).all() else None
        ref = next((t for t in (q, l, u, Q_values, A_values) if t is not None), None)
        ctx.layer, ctx.serial = layer, layer.serial
        ctx.device, ctx.solved, ctx.sizes = (None if ref is None else ref.device), layer.status == 1, (len(qp._Qview_keep[2]), len(qp._Apat[1]))
        to = dict(dtype=torch.float64, device=ref.device) if ref is not None else dict(dtype=torch.float64)
        return torch.from_numpy(r["x"]).to(**to), torch.from_numpy(r["y"]).to(**to)

    @staticmethod
    def backward(ctx, gx, gy):
        import numpy as np
        layer, qp = ctx.layer, ctx.layer.qp
        if layer.serial != ctx.serial:
            raise RuntimeError("WorkspaceQP.backward: the workspace has been solved again since this forward (solve %d, now %d); a workspace "
                               "holds one solution -- call backward before the next forward" % (ctx.serial, layer.serial))
        need = ctx.needs_input_grad[1:]                      # q, l, u, Q_values, A_values
        matrices = bool(need[3] or need[4])
        gxh = np.zeros(qp.n) if gx is None else np.ascontiguousarray(gx.detach().cpu().numpy(), np.float64)
        gyh = None if gy is None else np.ascontiguousarray(gy.detach().cpu().numpy(), np.float64)
        if ctx.solved:
            out = qp.adjoint(gxh, gyh, matrices=matrices, tol=layer.tol, max_sweeps=layer.max_sweeps)
        else:
            # the forward's solve did not end with QPDO_SOLVED (out of passes, infeasible): no adjoint call (the library refuses such a
            # workspace); the gradients are what FleetQP gives for an item with code 2 -- NaN, or zeros under on_failure = "zero"
            nan = lambda k: np.full(k, np.nan)
            out = dict(dq=nan(qp.n), dl=nan(qp.m), du=nan(qp.m), dQ_values=nan(ctx.sizes[0]), dA_values=nan(ctx.sizes[1]), status=np.array([2, 0, 0], np.int64))
        layer.adjoint_status = out["status"].copy()
        grads = []
        for want, key in zip(need, ("dq", "dl", "du", "dQ_values", "dA_values")):
            if not want:
                grads.append(None)
                continue
            g = out[key]
            if layer.on_failure == "zero" and out["status"][0] != 0:
                g = np.zeros_like(g)
            t = torch.from_numpy(np.ascontiguousarray(g))
            grads.append(t.to(ctx.device) if ctx.device is not None else t)
        return (None, *grads)


class WorkspaceQP(torch.nn.Module):
    """x, y = layer(q, l, u, Q_values=None, A_values=None): the solution of ONE QP held by a solver.QPDO workspace as a differentiable function
    of its data, at every size the workspace's direct solvers take (QPDO_LINSOLVE=dense or band -- the wide band, a variable order and coupling rows included; see qpdo_amd_adjoint for what is refused).
    qp: a solver.QPDO after setup.  q, l, u: tensors of n / m / m entries; Q_values / A_values: the stored values in the setup's pattern
    (qp._Qpat / qp._Apat: CSC column pointers and row indices; Q in the stype given to setup).  None inputs are left as they are in the
    workspace.  warm_start_last: start every solve from the previous finite solution.  on_failure: what the gradients hold when the adjoint
    was not delivered -- code 1 (not accepted), 3 (bad pivot), or 2: the forward's solve did not end with QPDO_SOLVED, in which case no
    adjoint call is made -- : "nan" or "zero", as in FleetQP.  layer.status: status_val of the last forward;
    layer.adjoint_status: (code, sweeps, active rows) of the last backward.  The workspace holds ONE solution: a backward that comes after
    another forward raises.
    layer.tangent(...) and layer.vjp_many(gx, gy) are the forward sensitivity (ONE qpdo_amd_tangent call) and R backward products (ONE
    qpdo_amd_adjoint call) of the most recent forward, R right-hand sides on one factorization; on_failure is applied per right-hand side and
    their status tensors are kept as layer.tangent_status and layer.vjp_status."""

    def __init__(self, qp, warm_start_last=True, on_failure="nan", tol=1e-9, max_sweeps=20):
        super().__init__()
        if on_failure not in ON_FAILURE:
            raise ValueError("on_failure: expected one of %r, got %r" % (ON_FAILURE, on_failure))
        self.qp, self.warm_start_last, self.on_failure, self.tol, self.max_sweeps = qp, bool(warm_start_last), on_failure, float(tol), int(max_sweeps)
        self.status, self.adjoint_status, self.serial, self._last = None, None, 0, None
        self.tangent_status, self.vjp_status = None, None

    def forward(self, q=None, l=None, u=None, Q_values=None, A_values=None):
        return _WorkspaceQPFunction.apply(self, q, l, u, Q_values, A_values)

    # ---- sensitivities of the most recent forward beside autograd: many right-hand sides per factorization ---------------------------------
    def _guard(self, what):
        if self.serial == 0:
            raise RuntimeError("WorkspaceQP.%s: no forward yet" % what)

    def _sensitivity(self, call, sizes, inputs):
        """the host round trip and on_failure of tangent / vjp_many.  call(**numpy inputs) -> the solver's dict; sizes: per
        gradient key its per-right-hand-side length (what a forward that did not end with QPDO_SOLVED is answered with, code 2)"""
        import numpy as np
        ref = next((t for t in inputs.values() if t is not None), None)
        host = {k: (None if t is None else np.ascontiguousarray(t.detach().cpu().numpy(), np.float64)) for k, t in inputs.items()}
        if self.status == 1:
            out = call(**host)
        else:
            lead = next(a for a in host.values() if a is not None).shape[:-1]
            out = {k: np.full(lead + (length,), np.nan) for k, length in sizes.items()}
            out.update(status=np.broadcast_to(np.array([2, 0, 0], np.int64), lead + (3,)).copy(), residual=np.full(lead, np.nan),
                       active=np.zeros(self.qp.m, np.int32))
        res = {}
        for k, v in out.items():
            if v is None:
                res[k] = None
                continue
            v = np.array(v)
            if k in sizes and self.on_failure == "zero":
                v[out["status"][..., 0] != 0] = 0.0
            t = torch.from_numpy(v)
            res[k] = t.to(ref.device) if k in sizes else t
        return res

    def tangent(self, tq=None, tl=None, tu=None, tQ_values=None, tA_values=None, tol=1e-9, max_sweeps=20):
        """The first-order change (dx, dy) of the most recent forward's x, y for a change of its inputs (solver.QPDO.tangent; tensors (L,) or
        (R, L)): a dict with dx, dy (on the inputs' device), active, status, residual.  Raises before any forward; the library refuses
        when the workspace has been updated or warm-started since that forward's solve."""
        if all(t is None for t in (tq, tl, tu, tQ_values, tA_values)):
            raise ValueError("no tangent passed: at least one of tq, tl, tu, tQ_values, tA_values is needed")
        self._guard("tangent")
        out = self._sensitivity(lambda **kw: self.qp.tangent(tol=tol, max_sweeps=max_sweeps, **kw), dict(dx=self.qp.n, dy=self.qp.m),
                                dict(tq=tq, tl=tl, tu=tu, tQ_values=tQ_values, tA_values=tA_values))
        self.tangent_status = out["status"].clone()
        return out

    def vjp_many(self, gx, gy=None, matrices=False, tol=1e-9, max_sweeps=20):
        """R vector-Jacobian products of the most recent forward at once (solver.QPDO.adjoint; gx (R, n), gy (R, m) or None): a dict with dq,
        dl, du, dQ_values, dA_values (matrices=True; else None), active, status, residual, each gradient with the leading R.  Raises before
        any forward; the library refuses when the workspace has been updated or warm-started since that forward's solve."""
        self._guard("vjp_many")
        qp = self.qp
        sizes = dict(dq=qp.n, dl=qp.m, du=qp.m)
        if matrices:
            sizes.update(dQ_values=len(qp._Qview_keep[2]), dA_values=len(qp._Apat[1]))
        out = self._sensitivity(lambda **kw: qp.adjoint(matrices=matrices, tol=tol, max_sweeps=max_sweeps, **kw), sizes, dict(gx=gx, gy=gy))
        if not matrices:
            out.update(dQ_values=None, dA_values=None)
        self.vjp_status = out["status"].clone()
        return out
