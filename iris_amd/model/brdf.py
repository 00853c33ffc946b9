"""BaseBRDF samplers (reference: model/brdf.py:20-136) as single fused gfx950 kernels."""
import torch
import torch.nn as nn

from .. import _lib as L


def diffuse_sampler(sample2, normal):
    """cosine-weighted direction around `normal` (model/brdf.py:20-34): the direction sample_diffuse draws"""
    return BaseBRDF().sample_diffuse(sample2, normal)[0]


def specular_sampler(sample2, roughness, wo, normal):
    """GGX half-vector sample reflected about it (model/brdf.py:36-59): the direction sample_specular draws"""
    return BaseBRDF().sample_specular(sample2, wo, normal, roughness)[0]


class BaseBRDF(nn.Module):
    """Parameter-free BRDF used by bake_shading (bake_shading.py:79)."""

    def __init__(self):
        super().__init__()

    def forward(self):
        pass

    def eval_diffuse(self, wi, normal):
        """(brdf Bx3, pdf Bx1), both relu(n.wi) / pi (model/brdf.py:70-76)"""
        import math
        wi = L.require_gpu(wi, torch.float32, "wi").reshape(-1, 3)
        normal = L.require_gpu(normal, torch.float32, "normal").reshape(-1, 3)
        pdf = ((normal * wi).sum(-1, keepdim=True)).relu() / math.pi
        return pdf.expand(wi.shape[0], 3), pdf

    def eval_specular(self, wi, wo, normal, roughness):
        """(brdf_spec0 Bx1, brdf_spec1 Bx1, pdf Bx1): the GGX lobe split by the two Schlick terms, F = ks F0 + F1 (model/brdf.py:90-110);
        D, G and the Fresnel terms are the HIP helpers of iris_amd.utils.ops.  No backward pass (the reference's version carries gradient to
        roughness, wi and normal): inputs that require grad raise instead of being cut off silently."""
        from ..utils import ops
        L.no_autograd("BaseBRDF.eval_specular", wi, wo, normal, roughness)
        wi = L.require_gpu(wi, torch.float32, "wi").reshape(-1, 3)
        wo = L.require_gpu(wo, torch.float32, "wo").reshape(-1, 3)
        normal = L.require_gpu(normal, torch.float32, "normal").reshape(-1, 3)
        half = torch.nn.functional.normalize(wi + wo, dim=-1)
        dot = lambda a, b: (a * b).sum(-1, keepdim=True).relu()
        n_l, n_v, v_h, n_h = dot(wi, normal), dot(wo, normal), dot(wo, half), dot(normal, half)
        if not torch.is_tensor(roughness):
            roughness = torch.tensor(float(roughness), device=wi.device)
        rough = roughness.detach().to(torch.float32).reshape(-1, 1) if roughness.numel() > 1 else roughness.detach().to(torch.float32).reshape(1, 1)
        D = ops.D_GGX(n_h, rough)
        pdf = D / (4 * v_h.clamp_min(1e-4)) * n_h
        DG = D * ops.G_Smith(n_v, n_l, rough)
        f0, f1 = ops.fresnelSchlick_sep(v_h)
        return DG * f0 / 4.0 * n_l, DG * f1 / 4.0 * n_l, pdf

    def sample_diffuse(self, sample2, normal):
        """Cosine-weighted direction, pdf = relu(n.wi)/pi, weight = 1 (model/brdf.py:78-88).  No backward pass."""
        L.no_autograd("BaseBRDF.sample_diffuse", sample2, normal)
        sample2 = L.require_gpu(sample2, torch.float32, "sample2").reshape(-1, 2)
        normal = L.require_gpu(normal, torch.float32, "normal").reshape(-1, 3)
        B = sample2.shape[0]
        wi = torch.empty(B, 3, device=sample2.device, dtype=torch.float32)
        pdf = torch.empty(B, 1, device=sample2.device, dtype=torch.float32)
        w = torch.empty(B, 3, device=sample2.device, dtype=torch.float32)
        with torch.cuda.device(sample2.device):
            L.check(L.lib().iris_sample_diffuse(L.ptr(sample2), L.ptr(normal), B, L.ptr(wi), L.ptr(pdf), L.ptr(w), L.stream()))
        return wi, pdf, w

    def sample_specular(self, sample2, wo, normal, roughness):
        """GGX half-vector sampling and the two Fresnel-split weights (model/brdf.py:112-136).
        roughness: python float or 0-d tensor (bake_shading.py:161 iterates a linspace), or one value per sample (Bx1).
        No backward pass (the reference's weights carry gradient to roughness; its sampled direction does not: model/brdf.py:46 uses .data)."""
        L.no_autograd("BaseBRDF.sample_specular", sample2, wo, normal, roughness)
        sample2 = L.require_gpu(sample2, torch.float32, "sample2").reshape(-1, 2)
        wo = L.require_gpu(wo, torch.float32, "wo").reshape(-1, 3)
        normal = L.require_gpu(normal, torch.float32, "normal").reshape(-1, 3)
        B = sample2.shape[0]
        each = None
        if isinstance(roughness, torch.Tensor):
            if roughness.numel() == 1:
                roughness = float(roughness.detach().float().cpu().item())
            else:                                           # one roughness per sample (what sample_brdf hands to specular_sampler)
                each = L.require_gpu(roughness.detach(), torch.float32, "roughness").reshape(-1)
                if each.shape[0] != B:
                    raise L.IrisError(f"sample_specular: {each.shape[0]} roughness values for {B} samples")
        wi = torch.empty(B, 3, device=sample2.device, dtype=torch.float32)
        pdf = torch.empty(B, 1, device=sample2.device, dtype=torch.float32)
        w0 = torch.empty(B, 1, device=sample2.device, dtype=torch.float32)
        w1 = torch.empty(B, 1, device=sample2.device, dtype=torch.float32)
        with torch.cuda.device(sample2.device):
            if each is not None:
                L.check(L.lib().iris_sample_specular_v(L.ptr(sample2), L.ptr(wo), L.ptr(normal), L.ptr(each), B, L.ptr(wi), L.ptr(pdf), L.ptr(w0), L.ptr(w1), L.stream()))
            else:
                L.check(L.lib().iris_sample_specular(L.ptr(sample2), L.ptr(wo), L.ptr(normal), roughness, B, L.ptr(wi), L.ptr(pdf), L.ptr(w0), L.ptr(w1), L.stream()))
        return wi, pdf, w0, w1

    @staticmethod
    def _mat(mat, dev):
        albedo = L.require_gpu(mat["albedo"].detach(), torch.float32, "mat['albedo']").reshape(-1, 3)
        rough = L.require_gpu(mat["roughness"].detach(), torch.float32, "mat['roughness']").reshape(-1)
        metal = L.require_gpu(mat["metallic"].detach(), torch.float32, "mat['metallic']").reshape(-1)
        return albedo, rough, metal

    def eval_brdf(self, wi, wo, normal, mat):
        """BRDF value (already multiplied by NoL) and the 50/50 diffuse + GGX sampling pdf (model/brdf.py:138-175).
        mat: {'albedo' Bx3, 'roughness' Bx1, 'metallic' Bx1}.  Returns brdf Bx3, pdf Bx1.  No backward pass: a material that requires
        grad raises (path_tracing_single differentiates w.r.t. the emitter radiance only, as train_emitter.py does)."""
        L.no_autograd("BaseBRDF.eval_brdf", wi, wo, normal, *[mat[k] for k in ("albedo", "roughness", "metallic")])
        wi = L.require_gpu(wi, torch.float32, "wi").reshape(-1, 3)
        wo = L.require_gpu(wo, torch.float32, "wo").reshape(-1, 3)
        normal = L.require_gpu(normal, torch.float32, "normal").reshape(-1, 3)
        albedo, rough, metal = self._mat(mat, wi.device)
        B = wi.shape[0]
        brdf = torch.empty(B, 3, device=wi.device, dtype=torch.float32)
        pdf = torch.empty(B, 1, device=wi.device, dtype=torch.float32)
        with torch.cuda.device(wi.device):
            L.check(L.lib().iris_eval_brdf(L.ptr(wi), L.ptr(wo), L.ptr(normal), L.ptr(albedo), L.ptr(rough), L.ptr(metal), B, L.ptr(brdf), L.ptr(pdf), L.stream()))
        return brdf, pdf

    def sample_brdf(self, sample1, sample2, wo, normal, mat):
        """importance sampling: diffuse lobe where sample1 > 0.5, GGX otherwise; returns wi Bx3, pdf Bx1, brdf/pdf Bx3
        (model/brdf.py:177-210).  No backward pass."""
        L.no_autograd("BaseBRDF.sample_brdf", wo, normal, *[mat[k] for k in ("albedo", "roughness", "metallic")])
        sample1 = L.require_gpu(sample1, torch.float32, "sample1").reshape(-1)
        sample2 = L.require_gpu(sample2, torch.float32, "sample2").reshape(-1, 2)
        wo = L.require_gpu(wo, torch.float32, "wo").reshape(-1, 3)
        normal = L.require_gpu(normal, torch.float32, "normal").reshape(-1, 3)
        albedo, rough, metal = self._mat(mat, wo.device)
        B = wo.shape[0]
        wi = torch.empty(B, 3, device=wo.device, dtype=torch.float32)
        pdf = torch.empty(B, 1, device=wo.device, dtype=torch.float32)
        w = torch.empty(B, 3, device=wo.device, dtype=torch.float32)
        with torch.cuda.device(wo.device):
            L.check(L.lib().iris_sample_brdf(L.ptr(sample1), L.ptr(sample2), L.ptr(wo), L.ptr(normal), L.ptr(albedo), L.ptr(rough), L.ptr(metal), B,
                                             L.ptr(wi), L.ptr(pdf), L.ptr(w), L.stream()))
        return wi, pdf, w


class _TcnnParams(nn.Module):
    """Stands where the reference has `self.mlp = tcnn.NetworkWithInputEncoding(...)`: it owns the ONE flat float32 parameter tensor tiny-cuda-nn's
    torch module registers as `params`, so the state-dict key is `mlp.params` as in the reference's checkpoints (refine_shading.py:84-89 strips the
    'material.' prefix and calls load_state_dict)."""

    def __init__(self, n):
        super().__init__()
        self.params = nn.Parameter(torch.zeros(n, dtype=torch.float32), requires_grad=False)


class _NGPForward(torch.autograd.Function):
    """`mlp.params` -> (albedo, roughness, metallic) for fixed positions: the forward is the inference path's iris_ngp_forward (the same bits), the backward
    iris_ngp_backward, which recomputes the forward from the positions (nothing is saved but the positions themselves)."""

    @staticmethod
    def forward(ctx, params, net, pos):
        ctx.net, ctx.pos = net, pos
        return net._run(pos)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_albedo, g_rough, g_metal):
        net, pos = ctx.net, ctx.pos
        N, dev = pos.shape[0], pos.device
        p = net.mlp.params
        grad = torch.zeros(p.numel(), device=dev, dtype=torch.float32)
        if N > 0:
            def cot(g, shape):
                return torch.zeros(shape, device=dev) if g is None else g.to(torch.float32).contiguous()
            g_albedo, g_rough, g_metal = cot(g_albedo, (N, 3)), cot(g_rough, (N,)), cot(g_metal, (N,))
            with torch.cuda.device(dev):
                nbytes = int(L.lib().iris_ngp_backward_workspace_bytes(N))
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                L.check(L.lib().iris_ngp_backward(net._handle(dev), L.ptr(pos), N, L.ptr(g_albedo), L.ptr(g_rough), L.ptr(g_metal), float(net.loss_scale),
                                                  L.ptr(grad), L.ptr(ws), nbytes, L.stream()))
        return grad, None, None


class NGPBRDF(BaseBRDF):
    """Hash-grid material network (model/brdf.py:213-260; the reference trains it in train_brdf_crf.py:163-207 and loads it frozen in refine_shading.py:83-92
    and train_emitter.py:67-77): HashGrid{32 levels x 2 features, 2^19 entries, base 16, x1.3} -> FullyFusedMLP{64 x 2, ReLU} -> sigmoid, as HIP kernels
    (level-major gathers; the perceptron on the matrix cores, iris_amd/csrc/iris_ngp.h).  tiny-cuda-nn is third party and CUDA only: its published
    algorithm is implemented, parity unpinned (oracle/ngp_torch.py).

    Training: with `mlp.params` on the GPU and requiring grad, forward runs under autograd and `backward()` fills `mlp.params.grad` (iris_ngp_backward:
    straight-through over every rounding to half, the forward recomputed from the positions, the matrices' gradient bitwise reproducible, the tables' gradient
    accumulated with float atomics).  `position` never gets a gradient -- the reference's positions come from `ray_intersect` and need none -- and a
    position that requires grad raises.  A frozen network (the constructor's state, and what load_ngpbrdf returns) takes the inference path unchanged.
    The constructor leaves the parameters all-zero and frozen, since existing callers load a checkpoint; a trainer calls init_parameters(), .to(device) and
    mlp.params.requires_grad_(True)."""

    # roughness = sigmoid(.) * 0.98 + 0.02 (model/brdf.py:258): never below 0.02 for finite network outputs.  path_tracing_single uses its SECOND evaluation of the
    # network (mat_next, utils/path_tracing.py:392) only for the test roughness > trace_roughness = 0.0 (model/emitter.py:209), whose outcome this bound decides:
    # iris_amd.utils.path_tracing skips that evaluation when the network declares a bound above trace_roughness (same outputs, bit for bit).
    roughness_min = 0.02
    # The backward multiplies the output-stage gradient by this before rounding it to half and divides the result by it again (tiny-cuda-nn's default): small
    # loss gradients do not flush to zero.  A scaled gradient beyond the half range (65504) becomes inf, and so does the parameter gradient, as in the library:
    # lower the value if the loss gradients are large.
    loss_scale = 128.0

    def __init__(self, voxel_min, voxel_max):
        super().__init__()
        self.voxel_min, self.voxel_max = float(voxel_min), float(voxel_max)
        self.mlp = _TcnnParams(int(L.lib().iris_ngp_n_params()))
        self._native = L.Native()

    def init_parameters(self, seed=1337):
        """tiny-cuda-nn's initial distributions, drawn from a torch generator on the CPU: tables U(-1e-4, 1e-4), the three matrices Xavier-uniform
        (+-sqrt(6 / (fan_in + fan_out)), the padded output matrix as 16 x 64).  The bits do not equal the library's RNG: parity unpinned.
        The constructor's all-zero network cannot be trained: with zero weights every gradient is zero, for ever."""
        import math
        g = torch.Generator().manual_seed(int(seed))
        p = self.mlp.params
        new = torch.empty(p.numel(), dtype=torch.float32)
        o = 0
        for rows, cols in ((64, 64), (64, 64), (16, 64)):
            a = math.sqrt(6.0 / (rows + cols))
            new[o:o + rows * cols] = (torch.rand(rows * cols, generator=g) * 2 - 1) * a
            o += rows * cols
        new[o:] = (torch.rand(p.numel() - o, generator=g) * 2 - 1) * 1e-4
        with torch.no_grad():
            p.copy_(new.to(p.device))
        return self

    def _handle(self, device):
        import ctypes as C
        p = self.mlp.params
        idx = L.device_index(device)
        n = self._native
        if n.ptr is not None and n.device == idx and n.keys[0].fresh(p):
            return n.ptr
        if p.is_cuda:
            # parameters that live on the GPU (a network being trained): ONE native object, refreshed on the device whenever the tensor has been written to
            # or swapped (L.tensor_key: every optimizer step bumps _version) -- no 112 MB round trip through the host
            if p.device.index != idx:
                raise L.IrisError(f"NGPBRDF: mlp.params is on {p.device}, position on cuda:{idx}")
            if n.ptr is None or n.device != idx:
                n = self._create(None, p.numel(), idx)
            src = p.detach()
            src = src if src.is_contiguous() and src.dtype == torch.float32 else src.to(torch.float32).contiguous()
            with torch.cuda.device(idx):
                L.check(L.lib().iris_ngp_set_params_dev(n.ptr, L.ptr(src), src.numel(), L.stream()))
        else:
            host = p.detach().to("cpu", torch.float32).contiguous()
            n = self._create(C.c_void_p(host.data_ptr()), host.numel(), idx)
        n.keys[0] = L.tensor_key(p)
        return n.ptr

    def _create(self, host_params, n_params, idx):
        import ctypes as C
        self._native.free()
        h = C.c_void_p()
        L.check(L.lib().iris_ngp_create(host_params, n_params, self.voxel_min, self.voxel_max, idx, C.byref(h)))
        self._native = L.Native(h, L.lib().iris_ngp_destroy, idx, (L.tensor_key(),))      # (the empty key: the parameters are not in yet)
        return self._native

    def adam_step_(self, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        """One torch.optim.Adam step of `mlp.params`, in place, which also writes the handle's half copy of the new parameters in the same pass
        (iris_ngp_adam_step): the next forward neither runs the cast kernel nor re-creates the handle.  grad, exp_avg, exp_avg_sq: float32, contiguous, on
        the parameters' device, of their length (exp_avg and exp_avg_sq are updated in place); step counts from 1.  What iris_amd.utils.optim.FusedAdam
        calls for a parameter of one of its `networks`; the refresh path (torch.optim.Adam, then a forward) stays as it is."""
        p = self.mlp.params
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise L.IrisError("NGPBRDF.adam_step_: mlp.params must be float32, contiguous and on a HIP device (net.to(device))")
        for name, t in (("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
            if not torch.is_tensor(t) or t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                raise L.IrisError(f"NGPBRDF.adam_step_: {name} must be a contiguous float32 tensor of {p.numel()} entries on {p.device}")
        idx = p.device.index
        n = self._native
        if n.ptr is None or n.device != idx:
            n = self._create(None, p.numel(), idx)
        with torch.cuda.device(idx):
            L.check(L.lib().iris_ngp_adam_step(n.ptr, L.ptr(p), L.ptr(grad), L.ptr(exp_avg), L.ptr(exp_avg_sq), p.numel(), int(step), float(lr),
                                               float(betas[0]), float(betas[1]), float(eps), float(weight_decay), L.stream()))
        torch.autograd.graph.increment_version(p)              # an in-place write, as far as autograd and every tensor_key are concerned
        n.keys[0] = L.tensor_key(p)                            # ... and the handle already holds the new values
        return self

    def _run(self, pos):
        N, dev = pos.shape[0], pos.device
        albedo = torch.empty(N, 3, device=dev); rough = torch.empty(N, device=dev); metal = torch.empty(N, device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib().iris_ngp_forward(self._handle(dev), L.ptr(pos), N, L.ptr(albedo), L.ptr(rough), L.ptr(metal), L.stream()))
        return albedo, rough, metal

    def forward(self, position):
        """position Bx3 (world space) -> {'albedo': Bx3, 'roughness': Bx1 in [0.02, 1], 'metallic': Bx1}  (model/brdf.py:243-260).
        Differentiable with respect to mlp.params when they require grad (and grad mode is on); never with respect to position, which raises if it
        requires grad: the reference's positions are ray_intersect's hit points."""
        L.no_autograd("NGPBRDF.forward", position)
        position = L.require_gpu(position, torch.float32, "position")
        shape = position.shape[:-1]
        pos = position.reshape(-1, 3)
        p = self.mlp.params
        if torch.is_grad_enabled() and p.requires_grad:
            if not p.is_cuda:
                raise L.IrisError("NGPBRDF.forward: mlp.params requires grad but lives on the CPU; move the network to the GPU first (net.to(device)): "
                                  "the backward pass and the parameter refresh run on the device")
            albedo, rough, metal = _NGPForward.apply(p, self, pos.detach())
        else:
            albedo, rough, metal = self._run(pos)
        return {"albedo": albedo.reshape(*shape, 3), "roughness": rough.reshape(*shape, 1), "metallic": metal.reshape(*shape, 1)}


def load_ngpbrdf(voxel_min, voxel_max, ckpt):
    """The reference's loading sequence (refine_shading.py:83-92): NGPBRDF(voxel_min, voxel_max), the checkpoint's 'state_dict' entries under 'material.'
    with the prefix stripped, load_state_dict, frozen."""
    from ..utils.stage import freeze, read_checkpoint
    net = NGPBRDF(voxel_min, voxel_max)
    net.load_state_dict(read_checkpoint(ckpt)["material"])
    freeze(net)
    return net
