"""The trainers' optimizer: torch.optim.Adam's arithmetic as one streaming HIP pass per parameter tensor (iris_amd/csrc/iris_optim.h).

The reference's stages call ``optim.Adam(self.parameters(), lr=, weight_decay=)`` (train_brdf_crf.py:106-114).  For the material network that is a dense
step over 27 963 328 parameters of which a batch touches a sliver: the step is memory traffic, and what follows it -- the refresh of the half copy the
forward reads -- is more of the same.  FusedAdam does the update in one kernel and, for the ``mlp.params`` of the networks it is told about, writes that
half copy in the same pass (``NGPBRDF.adam_step_``).

    optimizer = FusedAdam(list(material.parameters()) + list(model_crf.parameters()), lr=1e-3, networks=[material])

State and state dict are torch's (``step`` a 0-d float32 CPU tensor, ``exp_avg``, ``exp_avg_sq``): they load into ``torch.optim.Adam`` and back.
No amsgrad, no maximize; weight decay is L2 (added to the gradient).  The arithmetic, and in which precision the scalars are formed, is stated in
include/iris_hip.h and restated in tests/adam_ref.py.
"""
import torch

from .. import _lib as L


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, networks=()):
        if not 0.0 < lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 < eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # the keys of torch.optim.Adam's groups, so that either optimizer finds what it reads after loading the other's state dict
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None)
        super().__init__(params, defaults)
        self.networks = list(networks)
        for net in self.networks:
            if not hasattr(net, "adam_step_") or not hasattr(net, "mlp"):
                raise TypeError(f"networks: {type(net).__name__} has no adam_step_ (expected NGPBRDF)")

    @staticmethod
    def _check(p, grad):
        if grad.is_sparse:
            raise L.IrisError("FusedAdam: sparse gradients are not supported")
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise L.IrisError(f"FusedAdam: a parameter is {p.dtype} on {p.device}{'' if p.is_contiguous() else ', not contiguous'}: expected contiguous "
                              "float32 on a HIP device (there is no CPU path)")
        if grad.device != p.device or grad.dtype != torch.float32 or grad.shape != p.shape:
            raise L.IrisError(f"FusedAdam: a gradient is {grad.dtype} {tuple(grad.shape)} on {grad.device}, its parameter float32 {tuple(p.shape)} on {p.device}")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        nets = {id(net.mlp.params): net for net in self.networks}
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):          # (a loaded state dict may bring them)
                raise L.IrisError("FusedAdam: amsgrad, maximize and decoupled weight decay are not built")
            lr, (beta1, beta2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
            for p in group["params"]:
                if p.grad is None:
                    continue
                grad = p.grad
                self._check(p, grad)
                grad = grad if grad.is_contiguous() else grad.contiguous()
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                for name, t in (("exp_avg", m), ("exp_avg_sq", v)):
                    if t.device != p.device or t.dtype != torch.float32 or t.shape != p.shape or not t.is_contiguous():
                        raise L.IrisError(f"FusedAdam: state {name} is {t.dtype} {tuple(t.shape)} on {t.device}: expected the parameter's layout")
                step = int(state["step"]) + 1               # (a CPU tensor: no synchronisation; a state dict of torch's fused Adam holds it on the device)
                net = nets.get(id(p))
                if net is not None:
                    net.adam_step_(grad, m, v, step, lr, (beta1, beta2), eps, wd)
                else:
                    with torch.cuda.device(p.device):
                        L.check(L.lib().iris_adam_step(L.ptr(p), L.ptr(grad), L.ptr(m), L.ptr(v), p.numel(), step, lr, float(beta1), float(beta2), eps, wd,
                                                       L.stream()))
                    torch.autograd.graph.increment_version(p)
                state["step"] += 1
        return loss
