"""Deterministic stand-in for the reference's NGPBRDF (tiny-cuda-nn hash grid + MLP: third party):
same forward(position) -> {'albedo' Bx3, 'roughness' Bx1, 'metallic' Bx1} contract (model/brdf.py:243-260), closed form.
Evaluated with torch on the CPU everywhere (golden generation, oracle, GPU tests) so that all three see identical inputs."""
import numpy as np
import torch


class StubMaterial(torch.nn.Module):
    def forward(self, x):
        dev = x.device
        xc = x.detach().to("cpu", torch.float32)
        k = torch.tensor([1.3, 2.1, 0.7]); ph = torch.tensor([0.1, 0.5, 0.9])
        albedo = 0.5 + 0.4 * torch.sin(xc * k + ph)
        rough = 0.35 + 0.3 * torch.sin(xc[:, :1] * 1.7 + xc[:, 1:2] * 0.9)
        metal = 0.5 + 0.5 * torch.sin(xc[:, 2:3] * 2.3)
        return {"albedo": albedo.to(dev), "roughness": rough.to(dev), "metallic": metal.to(dev)}


def stub_material_np(position):
    out = StubMaterial()(torch.from_numpy(np.ascontiguousarray(position, dtype=np.float32)))
    return {k: v.numpy() for k, v in out.items()}


def material(voxel_min=None, voxel_max=None, ckpt=None):
    """factory with the signature `python -m iris_amd.refine_shading --material stub_material:material` expects (NGPBRDF(voxel_min, voxel_max))"""
    return StubMaterial()


class EdgeStubMaterial(StubMaterial):
    """StubMaterial with the values where the integrators branch planted at fixed fractions of the points: roughness exactly 0.02 and 1.0 (NGPBRDF's range,
    model/brdf.py:243-260) and float32(0.6) with its two float32 neighbours (eval_emitter's `roughness > trace_roughness`, model/emitter.py:209), metallic
    exactly 0 and 1.  The bucket of a point is a hash of its coordinate bits, so every evaluation of the same point -- GPU path or oracle -- gets the same row."""
    R06 = np.float32(0.6)
    ROUGH = (np.float32(0.02), np.float32(1.0), R06, np.nextafter(R06, np.float32(0.0)), np.nextafter(R06, np.float32(1.0)))
    METAL = (np.float32(0.0), np.float32(1.0))

    def forward(self, x):
        out = super().forward(x)
        bits = x.detach().to("cpu", torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        h = (bits[:, 0] * 73856093) ^ (bits[:, 1] * 19349663) ^ (bits[:, 2] * 83492791)
        h = (h ^ (h >> 13)) & 0xFFFF
        rough, metal = out["roughness"].to("cpu").clone(), out["metallic"].to("cpu").clone()
        for k, v in enumerate(self.ROUGH):                  # buckets 0..4 of 16: 5 / 16 of the points
            rough[h % 16 == k] = float(v)
        for k, v in enumerate(self.METAL):                  # buckets 0, 1 of 8 of an independent digit: 1 / 4 of the points
            metal[(h // 16) % 8 == k] = float(v)
        return {"albedo": out["albedo"], "roughness": rough.to(x.device), "metallic": metal.to(x.device)}


def edge_material_np(position):
    out = EdgeStubMaterial()(torch.from_numpy(np.ascontiguousarray(position, dtype=np.float32)))
    return {k: v.numpy() for k, v in out.items()}
