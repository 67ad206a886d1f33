"""csrc/weight_table.h - the one description of every checkpoint tensor (name, shape, how the handle packs it) that csrc/host.hip loops
over - compiled for the host with the address and undefined-behaviour sanitizers into a plain executable (tests/weight_table_main.cpp,
its own main) and printed for tiny, vits and vitl, each plain, with use_clstoken, with use_bn and with pe='rope'. The inventory must be
weights.state_dict_spec; every tensor must be packed, or be on the list below with its reason; the packed blocks must not overlap.
Nothing is loaded into Python."""
import math
import os
import re
import shutil
import subprocess

import pytest

from video_depth_anything_amd.config import get_config
from video_depth_anything_amd.weights import state_dict_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "weight_table_main.cpp")
INCLUDE = os.path.join(REPO, "video_depth_anything_amd", "csrc")
COMPILERS = ["g++", "/opt/rocm/llvm/bin/clang++", "clang++"]
VARIANTS = {"plain": {}, "clstoken": {"use_clstoken": True}, "bn": {"use_bn": True}, "rope": {"pe": "rope"}}
VECTORS = ("vec", "convt_bias", "geglu_bias")            # fp32, in the handle's `vec` map; every other kind is a matrix of the precision


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The sanitized executable, from the first compiler that builds one that runs."""
    out = str(tmp_path_factory.mktemp("weight_table") / "weight_table_main")
    tried = []
    for cxx in COMPILERS:
        if shutil.which(cxx) is None:
            tried.append(f"{cxx}: not found")
            continue
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", INCLUDE, SRC,
                            "-o", out], capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([out], capture_output=True).returncode == 0:
            return out
        tried.append(f"{cxx}: {r.stderr[-300:]}")
    pytest.skip("no host compiler links and runs a program with -fsanitize=address,undefined: " + "; ".join(tried))


def table(program, cfg):
    """(pads, {name: shape}, pack entries) as the program prints them for cfg."""
    args = [cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.features, *cfg.out_channels, cfg.num_frames, int(cfg.use_clstoken), int(cfg.use_bn),
            int(cfg.pe == "rope")]
    r = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    pads, spec, packs = None, [], []
    for line in r.stdout.splitlines():
        f = line.split(" ")
        if f[0] == "pads":
            pads = [int(v) for v in f[1:]]
        elif f[0] == "spec":
            spec.append((f[1], tuple(int(v) for v in f[2:])))
        else:
            assert f[0] == "pack" and len(f) == 10, line
            packs.append(dict(kind=f[1], key=f[2], name=f[3], **{k: int(v) for k, v in zip(("N", "K", "npad", "kpad", "row", "elems"), f[4:])}))
    return pads, spec, packs


def not_packed_from_the_table(cfg):
    """name -> why the table packs nothing from this tensor. Nothing else may be left out."""
    out = {"pretrained.pos_embed": "resampled to the clip's grid in vda_prepare",
           "pretrained.mask_token": "unused in inference",
           "head.scratch.output_conv2.2.bias": "one scalar, read to the host in vda_finalize_weights"}
    if cfg.use_bn:
        for name in state_dict_spec(cfg):
            if re.search(r"\.resConfUnit[12]\.bn[12]\.", name):
                out[name] = "BatchNorm tensor: folded into the conv before it by the derived step"
            elif re.search(r"\.resConfUnit[12]\.conv[12]\.(weight|bias)$", name):
                out[name] = "use_bn: packed by the derived step with its BatchNorm folded in"
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("encoder", ["tiny", "vits", "vitl"])
def test_the_table_is_the_inventory_and_packs_all_of_it_once(program, encoder, variant):
    cfg = get_config(encoder, **VARIANTS[variant])
    want = state_dict_spec(cfg)
    pads, spec, packs = table(program, cfg)
    assert pads == [(c + 63) // 64 * 64 for c in cfg.out_channels] + [(cfg.features // 2 + 31) // 32 * 32]

    # 1. the inventory: same names, same shapes, same count
    assert len(spec) == len(want) and dict(spec) == {k: tuple(v) for k, v in want.items()}

    # 2. every source is a tensor of the checkpoint; every tensor is packed or is on the list
    sources = {p["name"] for p in packs}
    assert sources <= set(want)
    assert set(want) - sources == set(not_packed_from_the_table(cfg))

    # 3. one block per key; only a `rows` key is shared, and its tensors tile it exactly
    by_key = {}
    for p in packs:
        by_key.setdefault((p["kind"] in VECTORS, p["key"]), []).append(p)
    assert len({key for _, key in by_key}) == len(by_key)              # (no name is in both of the handle's maps)
    for (_, key), ps in by_key.items():
        if ps[0]["kind"] != "rows":
            assert len(ps) == 1, key
            continue
        ps.sort(key=lambda p: p["row"])
        assert len({(p["kind"], p["npad"], p["kpad"], p["elems"]) for p in ps}) == 1, key
        assert [p["row"] for p in ps] == [sum(q["N"] for q in ps[:i]) for i in range(len(ps))], key
        assert sum(p["N"] for p in ps) == ps[0]["npad"], key
    assert sum(len(ps) > 1 for ps in by_key.values()) == 8             # to_q | to_k | to_v of the 4 x 2 temporal attention blocks

    # 4. true sizes are the shape's, padded sizes hold them, and the block is the kernel layout's size
    for p in packs:
        shape, kind = want[p["name"]], p["kind"]
        N = shape[0] if len(shape) >= 2 else 1
        assert (p["N"], p["N"] * p["K"]) == (N, math.prod(shape)), p
        assert p["row"] == 0 or kind == "rows", p
        if kind == "conv3":
            assert shape[2:] == (3, 3) and p["npad"] >= shape[0] and p["kpad"] >= shape[1] and p["elems"] == p["npad"] * 9 * p["kpad"], p
        elif kind == "convt":                                           # [Ci, Co, k, k], one padded width for both
            assert shape[2] == shape[3] and p["npad"] == p["kpad"] >= max(shape[:2]) and p["elems"] == shape[2] ** 2 * p["npad"] ** 2, p
        elif kind == "convt_bias":                                      # one padded copy per tap of the ConvTranspose it belongs to
            taps = math.prod(want[p["name"][:-len("bias")] + "weight"][2:])
            assert p["kpad"] >= p["K"] and p["npad"] == taps * p["kpad"] == p["elems"], p
        elif kind in ("geglu", "geglu_bias"):                           # interleaved, never padded: whole 32-row groups
            assert (p["npad"], p["kpad"]) == (p["N"], p["K"]) and shape[0] % 32 == 0 and p["elems"] == math.prod(shape), p
        else:
            assert kind in ("vec", "mat", "rows") and p["npad"] >= p["N"] and p["kpad"] >= p["K"] and p["elems"] == p["npad"] * p["kpad"], p
            assert kind != "vec" or p["npad"] == 1, p
    # the patch embedding's K is its shape's 3 x 14 x 14, padded to the GEMM's 640
    patch = [p for p in packs if p["key"] == "patch.w"]
    assert len(patch) == 1 and (patch[0]["K"], patch[0]["kpad"]) == (588, 640)
