"""KAN variant: efficient-KAN's ``KAN`` / ``KANLinear`` (kan.py:6-285, used by
run.py:92-93 as ``KAN([1, H, H, 1])``) with the reference's constructor API, parameter and
buffer names (``layers.{l}.base_weight``, ``.spline_weight``, ``.spline_scaler``, ``.grid``) and
init, computing on the gfx950 path (kan.hip through the C-ABI siren_kan_*).

Init runs the same torch calls in the same order as the reference (kaiming-uniform base
weight, a uniform-noise curve fitted by least squares onto the B-spline basis, kaiming-uniform
scaler), so ``torch.manual_seed(s)`` gives bit-identical parameters.  The B-spline basis used
for that fit is the Cox-de Boor recursion of kan.py:94-104, vectorised over knots.

Supported: spline_order 3 with any grid_size from 1 to 64 (run.py uses 5; the other sizes run the
any-grid-size kernels of kan.hip), SiLU base activation, standalone spline scaler.  ``KAN.forward`` and ``KANLinear.forward`` are differentiable
(``_KanFunction``: siren_kan_forward, then siren_kan_backward for any upstream gradient, into the
parameters and, when asked for, the input), so a user loop with ``loss.backward()`` and
``torch.optim`` trains them as it trains the reference's modules (kan.py:153-166, 268-273); the
fused fit goes through ``KanEngine`` / ``run.train(arch='kan')``.  ``KANLinear.update_grid`` /
``KAN.forward(x, update_grid=True)`` (kan.py:168-215, :274-279) run on the HIP path too
(siren_kan_regrid_*: knots, per-input Gram sums in fp64, Cholesky refit) at grid_size 5, the size at
which they are checked against the reference; ``regularization_loss``
(kan.py:217-237, :281-285) is the reference's torch expression on the parameters.

``KANLinear.regrid`` / ``KAN.regrid`` (no counterpart in the reference) return a new layer / model on a
grid of another size, 1 to 64, fitted to this one over a batch (the same three steps, ``_refit``, with
Gram matrices of (Gn+3)^2 and (Gn+3) x (Go+3)): the step of a coarse-to-fine grid
curriculum, ``run.train(kan_prev_grid_size=...)``.  They refit the unscaled coefficients and keep the
layer's function, unlike update_grid, which stores a scaled fit undivided.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import SirenKanBatch, SirenKanGrads, SirenKanNet, check, ptr


def bspline_bases(x: torch.Tensor, knots: torch.Tensor, order: int) -> torch.Tensor:
    """(batch, in) inputs on per-input knots (in, G) -> (batch, in, G - 1 - order) bases, by the
    Cox-de Boor recursion with kan.py:94-104's operation order."""
    x = x.unsqueeze(-1)
    lo, hi = knots[:, :-1], knots[:, 1:]
    b = ((x >= lo) & (x < hi)).to(x.dtype)
    for k in range(1, order + 1):
        left = (x - knots[:, :-(k + 1)]) / (knots[:, k:-1] - knots[:, :-(k + 1)]) * b[:, :, :-1]
        right = (knots[:, k + 1:] - x) / (knots[:, k + 1:] - knots[:, 1:(-k)]) * b[:, :, 1:]
        b = left + right
    return b.contiguous()


class KANLinear(torch.nn.Module):
    """kan.py:6-166 (parameters, buffer and init; forward on the HIP path via KAN)."""

    def __init__(self, in_features, out_features, grid_size=5, spline_order=3, scale_noise=0.1,
                 scale_base=1.0, scale_spline=1.0, enable_standalone_scale_spline=True,
                 base_activation=torch.nn.SiLU, grid_eps=0.02, grid_range=[-1, 1]):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.grid_size, self.spline_order = grid_size, spline_order
        step = (grid_range[1] - grid_range[0]) / grid_size
        knots = torch.arange(-spline_order, grid_size + spline_order + 1) * step + grid_range[0]
        self.register_buffer("grid", knots.expand(in_features, -1).contiguous())
        self.base_weight = torch.nn.Parameter(torch.Tensor(out_features, in_features))
        self.spline_weight = torch.nn.Parameter(torch.Tensor(out_features, in_features, grid_size + spline_order))
        if enable_standalone_scale_spline:
            self.spline_scaler = torch.nn.Parameter(torch.Tensor(out_features, in_features))
        self.scale_noise, self.scale_base, self.scale_spline = scale_noise, scale_base, scale_spline
        self.enable_standalone_scale_spline = enable_standalone_scale_spline
        self.base_activation = base_activation()
        self.grid_eps = grid_eps
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.kaiming_uniform_(self.base_weight, a=math.sqrt(5) * self.scale_base)
        with torch.no_grad():
            g = self.grid_size
            noise = (torch.rand(g + 1, self.in_features, self.out_features) - 1 / 2) * self.scale_noise / g
            interior = self.grid.T[self.spline_order:-self.spline_order]
            coeff = self.curve2coeff(interior, noise)
            self.spline_weight.data.copy_((1.0 if self.enable_standalone_scale_spline else self.scale_spline)
                                          * coeff)
            if self.enable_standalone_scale_spline:
                torch.nn.init.kaiming_uniform_(self.spline_scaler, a=math.sqrt(5) * self.scale_spline)

    def b_splines(self, x: torch.Tensor) -> torch.Tensor:
        return bspline_bases(x, self.grid, self.spline_order)

    def curve2coeff(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """Least-squares spline coefficients (out, in, coeff) of curves y (batch, in, out)
        sampled at x (batch, in) -- kan.py:106-135."""
        sol = torch.linalg.lstsq(self.b_splines(x).transpose(0, 1), y.transpose(0, 1)).solution
        return sol.permute(2, 0, 1).contiguous()

    @property
    def scaled_spline_weight(self):
        s = self.spline_scaler.unsqueeze(-1) if self.enable_standalone_scale_spline else 1.0
        return self.spline_weight * s

    def forward(self, x: torch.Tensor):
        """kan.py:153-166: (..., in) -> (..., out), a one-layer KAN on the HIP path (differentiable)."""
        _hip_check_layer(self)
        return _kan_apply([self.in_features, self.out_features], [self], x,
                          [self.base_weight, self.spline_weight, self.spline_scaler])

    def _refit(self, x: torch.Tensor, g_new: int, margin, chunk, scaled: bool, who: str, outcome: str):
        """The steps update_grid and regrid share (siren_kan_regrid_*): the order statistics of x
        (batch, in), the knots of a grid of `g_new` intervals from them, the Gram sums of the new and
        the old bases in row chunks, and the refit of spline_weight (times spline_scaler when `scaled`)
        on the new knots.  Returns (grid_new, spline_weight_new) and writes nothing of the layer's; a
        rank-deficient input raises SirenError in the caller's words `who` and `outcome`."""
        if not x.is_cuda:
            raise RuntimeError(f"KANLinear.{who} runs on the HIP path only (CUDA tensors)")
        if x.dim() != 2 or x.size(1) != self.in_features:
            raise ValueError(f"{who}: x must be (batch, {self.in_features})")
        lib, dev = _lib.load(), x.device
        s = torch.cuda.current_stream(dev).cuda_stream
        n_in, n_out, rows, g_old = self.in_features, self.out_features, x.size(0), self.grid_size
        xs = x.detach().float().contiguous()
        # order statistics: any exact selection will do; the indices are the reference's own call
        idx = torch.linspace(0, rows - 1, g_new + 1, dtype=torch.int64)
        q = torch.sort(xs, dim=0)[0][idx.to(dev)].contiguous()
        grid_old = self.grid.detach().to(dev, torch.float32).contiguous()
        grid_new = torch.empty(n_in, g_new + 7, dtype=torch.float32, device=dev)
        check(lib.siren_kan_regrid_knots(ptr(q), n_in, g_new, float(margin), float(self.grid_eps), ptr(grid_new), s),
              "siren_kan_regrid_knots")
        rows_c = max(1, min(int(chunk), rows))
        ws = torch.empty(int(lib.siren_kan_regrid_workspace_bytes(rows_c, n_in, g_old, g_new)), dtype=torch.uint8,
                         device=dev)
        gram = torch.empty(n_in * (g_new + 3) * (g_new + g_old + 6), dtype=torch.float64, device=dev)
        for lo in range(0, rows, rows_c):
            hi = min(rows, lo + rows_c)
            check(lib.siren_kan_regrid_gram(ptr(xs[lo:hi]), hi - lo, n_in, g_old, g_new, ptr(grid_old), ptr(grid_new),
                                            int(lo > 0), ptr(gram), ptr(ws), s), "siren_kan_regrid_gram")
        sw = self.spline_weight.detach().to(dev, torch.float32).contiguous()
        scaler = self.spline_scaler.detach().to(dev, torch.float32).contiguous() if scaled else None
        sw_new = torch.empty(n_out, n_in, g_new + 3, dtype=torch.float32, device=dev)
        status = torch.empty(2, dtype=torch.int32, device=dev)
        check(lib.siren_kan_regrid_refit(ptr(gram), n_in, n_out, g_old, g_new, ptr(sw), ptr(scaler), ptr(sw_new),
                                         ptr(status), s), "siren_kan_regrid_refit")
        bad, first = status.tolist()  # the one host synchronisation: this is not a per-step call
        if bad:
            raise _lib.SirenError(
                f"{who}: the refit of input {first} is rank deficient ({bad} input(s) in all: a constant input, or "
                f"fewer than {g_new + 3} distinct useful samples); {outcome}")
        return grid_new, sw_new

    @torch.no_grad()
    def update_grid(self, x: torch.Tensor, margin=0.01, chunk: int = 1 << 20):
        """kan.py:168-215 on the HIP path: new knots from the order statistics of x (batch, in), then
        the curves refitted on them over the batch -- through the Gram matrices of the bases per input
        (``_refit`` at the layer's own grid size), not the reference's (batch, in, out) intermediate
        and lstsq.  Like the reference the refit targets the scaled curves and stores the result in
        spline_weight undivided.  `grid` and `spline_weight` are written in place, and only once the
        refit succeeded: an input whose Gram matrix is rank deficient (a constant input, fewer than
        8 distinct useful samples) raises SirenError and leaves the layer as it was."""
        _hip_check_layer(self)
        _update_grid_check(self.grid_size)
        grid_new, sw_new = self._refit(x, self.grid_size, margin, chunk, True, "update_grid", "the layer is unchanged")
        self.grid.copy_(grid_new)
        self.spline_weight.data.copy_(sw_new)

    @torch.no_grad()
    def regrid(self, x: torch.Tensor, grid_size: int, margin=0.01, chunk: int = 1 << 20) -> "KANLinear":
        """A new layer at `grid_size` (1 to 64, the layer's own size included) that computes this
        layer's function on knots taken from x (batch, in): the knots are update_grid's (kan.py:183-212
        with `grid_size` for the grid size), and the curves are refitted on them by least squares over
        the batch through the Gram matrices of the new and the old bases (``_refit``).
        ``base_weight`` and ``spline_scaler`` are copied and ``spline_weight`` is refitted from the
        UNSCALED coefficients; by linearity the new layer's scaled curves are then the least-squares
        fit of this layer's scaled curves, so the layer's function is kept up to that fit.  This is
        deliberately not update_grid's quirk (kan.py:175, :215), which fits the scaled curves and
        stores the result undivided, scaling the curves by spline_scaler once more.  `self` is never
        modified; a rank-deficient input (a constant input, fewer than grid_size + 3 distinct useful
        samples) raises SirenError and returns nothing.  Not differentiable."""
        _hip_check_layer(self)
        _hip_check_grid(grid_size, self.spline_order)
        grid_new, sw_new = self._refit(x, int(grid_size), margin, chunk, False, "regrid", "no layer is returned")
        new = _blank_layer(self, int(grid_size)).to(x.device)
        new.grid.copy_(grid_new)
        new.base_weight.data.copy_(self.base_weight.detach())
        new.spline_scaler.data.copy_(self.spline_scaler.detach())
        new.spline_weight.data.copy_(sw_new)
        return new

    def regularization_loss(self, regularize_activation=1.0, regularize_entropy=1.0):
        """kan.py:217-237: the L1 / entropy surrogate on the spline weights (differentiable torch ops)."""
        mean_abs = self.spline_weight.abs().mean(-1)
        activation = mean_abs.sum()
        p = mean_abs / activation
        entropy = -torch.sum(p * p.log())
        return regularize_activation * activation + regularize_entropy * entropy


def _hip_check_grid(grid_size, spline_order):
    if spline_order != 3:
        raise NotImplementedError(f"HIP KAN path: spline_order=3 only (got {spline_order})")
    if not 1 <= int(grid_size) <= _lib.KAN_MAX_GRID or int(grid_size) != grid_size:
        raise NotImplementedError(f"HIP KAN path: grid_size from 1 to {_lib.KAN_MAX_GRID} (got {grid_size})")


def _blank_layer(src: "KANLinear", grid_size: int) -> "KANLinear":
    """A KANLinear with src's shape and settings at another grid size, for regrid to fill; its
    constructor's random init is drawn from a forked generator, so the caller's stream is untouched."""
    with torch.random.fork_rng(devices=[]):
        return KANLinear(src.in_features, src.out_features, grid_size=grid_size, spline_order=src.spline_order,
                         scale_noise=src.scale_noise, scale_base=src.scale_base, scale_spline=src.scale_spline,
                         grid_eps=src.grid_eps)


def _update_grid_check(grid_size):
    if grid_size != 5:
        raise NotImplementedError(
            f"update_grid is checked against the reference at grid_size=5 only; grid_size={grid_size} trains, "
            "infers and regrids on the HIP path but cannot update its grid in place")


def _hip_check_layer(lay: "KANLinear"):
    _hip_check_grid(lay.grid_size, lay.spline_order)
    if not lay.enable_standalone_scale_spline or not isinstance(lay.base_activation, torch.nn.SiLU):
        raise NotImplementedError("HIP KAN path: SiLU base and a standalone spline scaler")
    # kan.hip finds a basis span by counting knots <= x, which equals kan.py:94-96's span predicate
    # for non-decreasing knots (kan.py's grids always are; checked once per grid version)
    key = (lay.grid.data_ptr(), lay.grid._version)
    if getattr(lay, "_knots_checked", None) != key:
        g = lay.grid
        if not bool((g[:, 1:] >= g[:, :-1]).all()):
            raise NotImplementedError("HIP KAN path: every input's knots must be non-decreasing")
        lay._knots_checked = key


def _kan_splits(rows: int) -> int:
    return max(1, min(256, rows // 2048))


def _net(widths, layers, params) -> SirenKanNet:
    n = SirenKanNet()
    n.n_layers, n.grid_size = len(layers), layers[0].grid_size
    if any(lay.grid_size != n.grid_size for lay in layers):
        raise NotImplementedError("HIP KAN path: one grid_size for every layer of a stack")
    for l, w in enumerate(widths):
        n.width[l] = w
    for l, lay in enumerate(layers):
        n.grid[l] = ptr(lay.grid)
        n.base_w[l], n.spline_w[l], n.scaler[l] = (ptr(t) for t in params[3 * l:3 * l + 3])
    return n


class _KanFunction(torch.autograd.Function):
    """HIP forward (siren_kan_forward) and backward (siren_kan_backward, any upstream gradient) of
    a KANLinear stack; params = (base_weight, spline_weight, spline_scaler) per layer."""

    @staticmethod
    def forward(ctx, widths, layers, x, *params):
        lib = _lib.load()
        if not x.is_cuda:
            raise RuntimeError("KAN runs on the HIP path only (CUDA tensors)")
        dev = x.device
        p = [t.detach().contiguous().float() for t in params]
        net = _net(widths, layers, p)
        xs = x.detach().reshape(-1, widths[0]).contiguous().float()
        rows = xs.shape[0]
        splits = _kan_splits(rows)
        ws = torch.empty(int(lib.siren_kan_workspace_floats(ctypes.byref(net), rows, splits)), device=dev)
        out = torch.empty(rows, widths[-1], dtype=torch.float32, device=dev)
        g = torch.zeros(rows, widths[-1], dtype=torch.float32, device=dev)
        b = SirenKanBatch()
        b.rows, b.n_valid, b.n_total, b.splits, b.zero_grads = rows, 0, 1.0, splits, 0
        b.coords, b.target, b.out, b.g, b.ws = ptr(xs), 0, ptr(out), ptr(g), ptr(ws)
        check(lib.siren_kan_forward(ctypes.byref(net), ctypes.byref(b), torch.cuda.current_stream(dev).cuda_stream),
              "siren_kan_forward")
        # the input and parameters go through save_for_backward so that torch's version counter
        # catches an in-place change between forward and backward (the workspace holds state
        # computed from them, e.g. the combined spline_w * scaler weights); the rest is non-tensor
        # state and the workspace
        ctx.save_for_backward(x, *params)
        ctx.keep = (net, b, ws, xs, g, p, x.shape, [t.shape for t in params])
        return out.reshape(*x.shape[:-1], widths[-1])

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        _ = ctx.saved_tensors  # raises if x or a parameter was modified in place since the forward
        if ctx.keep is None:
            raise RuntimeError("KAN HIP backward: the forward's workspace is consumed by the first backward; "
                               "run the forward again instead of backward(retain_graph=True) twice")
        net, b, ws, xs, g, p, xshape, shapes = ctx.keep
        dev = xs.device
        g.copy_(grad_out.reshape(g.shape).float())
        grads = [torch.zeros(shp, dtype=torch.float32, device=dev) for shp in shapes]
        gs = SirenKanGrads()
        for l in range(len(shapes) // 3):
            gs.base_w[l], gs.spline_w[l], gs.scaler[l] = (ptr(t) for t in grads[3 * l:3 * l + 3])
        gx = torch.empty_like(xs) if ctx.needs_input_grad[2] else None
        check(lib.siren_kan_backward(ctypes.byref(net), ctypes.byref(gs), ctypes.byref(b), ptr(gx),
                                     torch.cuda.current_stream(dev).cuda_stream), "siren_kan_backward")
        ctx.keep = None
        return (None, None, None if gx is None else gx.reshape(xshape), *grads)


def _kan_apply(widths, layers, x, params):
    return _KanFunction.apply(list(widths), list(layers), x, *params)


class KAN(torch.nn.Module):
    """kan.py:169-285: a stack of KANLinear layers over layers_hidden widths."""

    def __init__(self, layers_hidden, grid_size=5, spline_order=3, scale_noise=0.1, scale_base=1.0,
                 scale_spline=1.0, base_activation=torch.nn.SiLU, grid_eps=0.02, grid_range=[-1, 1]):
        super().__init__()
        self.grid_size, self.spline_order = grid_size, spline_order
        self.widths = list(layers_hidden)
        self.layers = torch.nn.ModuleList(
            KANLinear(i, o, grid_size=grid_size, spline_order=spline_order, scale_noise=scale_noise,
                      scale_base=scale_base, scale_spline=scale_spline, base_activation=base_activation,
                      grid_eps=grid_eps, grid_range=grid_range)
            for i, o in zip(layers_hidden, layers_hidden[1:]))

    def hip_check(self):
        _hip_check_grid(self.grid_size, self.spline_order)
        if len(self.layers) > _lib.KAN_MAX_LAYERS or self.widths[-1] != 1:
            raise NotImplementedError(f"HIP KAN path: <= {_lib.KAN_MAX_LAYERS} layers, last width 1")
        for lay in self.layers:
            _hip_check_layer(lay)
            if lay.grid_size != self.grid_size:
                raise NotImplementedError("HIP KAN path: one grid_size for every layer of a stack")

    def param_index(self):
        pos = {n: k for k, (n, _) in enumerate(self.named_parameters())}
        return [(pos[f"layers.{l}.base_weight"], pos[f"layers.{l}.spline_weight"], pos[f"layers.{l}.spline_scaler"])
                for l in range(len(self.layers))]

    def make_net(self, tensors=None) -> SirenKanNet:
        """C-ABI view of the layers; `tensors` overrides the parameters (list in
        named_parameters order, e.g. views of a flat vector)."""
        self.hip_check()
        n = SirenKanNet()
        n.n_layers, n.grid_size = len(self.layers), self.grid_size
        for l, w in enumerate(self.widths):
            n.width[l] = w
        params = tensors if tensors is not None else [p for _, p in self.named_parameters()]
        for l, (ib, isp, isc) in enumerate(self.param_index()):
            n.grid[l] = ptr(self.layers[l].grid)
            n.base_w[l], n.spline_w[l], n.scaler[l] = ptr(params[ib]), ptr(params[isp]), ptr(params[isc])
        return n

    def forward(self, x: torch.Tensor, update_grid=False):
        """kan.py:268-273: (..., in) CUDA coords -> (..., out).  Differentiable when autograd needs
        it (siren_kan_forward + siren_kan_backward); chunked HIP inference otherwise."""
        if not x.is_cuda:
            raise RuntimeError("KAN.forward runs on the HIP path only (CUDA tensors)")
        self.hip_check()
        if update_grid:
            _update_grid_check(self.grid_size)
            # kan.py:274-279: per layer, update_grid(x) then x = layer(x); the layer forwards run the
            # lone-layer route in row chunks, so the output is the updated model's (not differentiable:
            # the reference's update_grid is @torch.no_grad too, and the refit moves the parameters)
            lead = x.shape[:-1]
            with torch.no_grad():
                h = x.detach().reshape(-1, self.widths[0]).float().contiguous()
                for lay in self.layers:
                    lay.update_grid(h)
                    h = layer_forward(lay, h)
            return h.reshape(*lead, self.widths[-1])
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            params = [t for lay in self.layers for t in (lay.base_weight, lay.spline_weight, lay.spline_scaler)]
            return _kan_apply(self.widths, self.layers, x, params)
        lead = x.shape[:-1]
        with torch.no_grad():
            out = kan_forward(self, x.reshape(-1, self.widths[0]), x.device)
        return out.reshape(*lead, 1)

    @torch.no_grad()
    def regrid(self, x: torch.Tensor, grid_size: int, margin=0.01, chunk: int = 1 << 20) -> "KAN":
        """A new model at `grid_size` fitted to this one over the coordinates x (..., in), in the order
        of kan.py:274-279: per layer ``KANLinear.regrid`` on the layer's input h, then h = new_layer(h),
        so a later layer's knots come from the activations of the already refitted layers before it.
        This model is not modified and nothing is differentiable; a ``KanEngine`` is sized by the
        grid, so build a new engine from the returned model."""
        _hip_check_grid(grid_size, self.spline_order)
        if not x.is_cuda:
            raise RuntimeError("KAN.regrid runs on the HIP path only (CUDA tensors)")
        h = x.detach().reshape(-1, self.widths[0]).float().contiguous()
        layers = []
        for lay in self.layers:
            layers.append(lay.regrid(h, grid_size, margin=margin, chunk=chunk))
            h = layer_forward(layers[-1], h)
        new = KAN.__new__(KAN)  # the constructor would draw and fit an init for every layer
        torch.nn.Module.__init__(new)
        new.grid_size, new.spline_order, new.widths = int(grid_size), self.spline_order, list(self.widths)
        new.layers = torch.nn.ModuleList(layers)
        return new

    def regularization_loss(self, regularize_activation=1.0, regularize_entropy=1.0):
        """kan.py:281-285: the layers' regularisation losses summed."""
        return sum(lay.regularization_loss(regularize_activation, regularize_entropy) for lay in self.layers)


def kan_forward(model: KAN, coords: torch.Tensor, device, chunk: int = 1 << 20, net=None) -> torch.Tensor:
    lib = _lib.load()
    net = net or model.make_net()
    n = coords.shape[0]
    rows = max(1, min(chunk, n))
    ws = torch.empty(int(lib.siren_kan_workspace_floats(ctypes.byref(net), rows, 1)), device=device)
    out = torch.empty(n, dtype=torch.float32, device=device)
    g = torch.empty(rows, dtype=torch.float32, device=device)
    o = torch.empty(rows, dtype=torch.float32, device=device)
    s = torch.cuda.current_stream(device).cuda_stream
    for lo in range(0, n, rows):
        hi = min(n, lo + rows)
        c = coords[lo:hi].to(device, torch.float32).contiguous()
        b = SirenKanBatch()
        b.rows, b.n_valid, b.n_total, b.splits, b.zero_grads = hi - lo, 0, 1.0, 1, 0
        b.coords, b.target, b.out, b.g, b.ws = ptr(c), 0, ptr(o), ptr(g), ptr(ws)
        check(lib.siren_kan_forward(ctypes.byref(net), ctypes.byref(b), s), "siren_kan_forward")
        out[lo:hi] = o[:hi - lo]
    return out


def layer_forward(lay: KANLinear, x: torch.Tensor, chunk: int = 1 << 18) -> torch.Tensor:
    """(rows, in) -> (rows, out) of one layer by siren_kan_forward on a one-layer net, in row chunks
    (inference; the same kernels, row by row the same bits, as the layer inside a stack)."""
    lib, dev = _lib.load(), x.device
    widths = [lay.in_features, lay.out_features]
    net = _net(widths, [lay], [lay.base_weight.detach(), lay.spline_weight.detach(), lay.spline_scaler.detach()])
    n = x.shape[0]
    rows = max(1, min(chunk, n))
    ws = torch.empty(int(lib.siren_kan_workspace_floats(ctypes.byref(net), rows, 1)), device=dev)
    out = torch.empty(n, widths[1], dtype=torch.float32, device=dev)
    g = torch.empty(rows, widths[1], dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    for lo in range(0, n, rows):
        hi = min(n, lo + rows)
        b = SirenKanBatch()
        b.rows, b.n_valid, b.n_total, b.splits, b.zero_grads = hi - lo, 0, 1.0, 1, 0
        b.coords, b.target, b.out, b.g, b.ws = ptr(x[lo:hi]), 0, ptr(out[lo:hi]), ptr(g), ptr(ws)
        check(lib.siren_kan_forward(ctypes.byref(net), ctypes.byref(b), s), "siren_kan_forward")
    return out


def make_kan_grads(model: KAN, views, sse_ptr: int, flat: torch.Tensor, flat_len: int) -> SirenKanGrads:
    g = SirenKanGrads()
    for l, (ib, isp, isc) in enumerate(model.param_index()):
        g.base_w[l], g.spline_w[l], g.scaler[l] = ptr(views[ib]), ptr(views[isp]), ptr(views[isc])
    g.sse, g.flat, g.flat_len = sse_ptr, ptr(flat), flat_len
    return g
