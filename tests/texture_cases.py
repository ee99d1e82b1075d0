"""
The probe table of the GLSL 3.30 §8.7 texture lookups of translated fragments (csrc/jit_runtime.hpp): the sampled textures, the
coordinates, lods, gradients and offsets, the probe fragments and the expected values by tests/texture_ref.py. Shared by
tests/test_host_texture.py (x86 host build) and tests/test_gpu_texture.py (gfx950).

A probe reads its operands from two RGBA32F textures (texel = pixel, NEAREST) and writes the lookup's four floats to an RGBA32F
target of 16 x 16, one row of the table per pixel; the uniform `form` selects the function. Offsets have to be constant expressions
in GLSL, so every (function, offset) pair is a form of its own. The sampled textures are a reduction of the full product of sizes,
formats, wraps and modes: see configs().
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import binding as O
from tests import texture_ref as R

F = np.float32
WIDTH = HEIGHT = 16
ROWS = WIDTH*HEIGHT

SIZES = [(8, 8), (5, 3), (16, 4), (1, 1)]                            # (width, height): levels 4, 3 (5x3, 2x1, 1x1), 5, 1
FORMATS = {"rgba8": (np.uint8, 4), "rgb8": (np.uint8, 3), "r32f": (np.float32, 1), "rg16f": (np.float16, 2)}
WRAPS = [(True, True), (False, False), (True, False), (False, True)]              # (repeat_x, repeat_y)
MODES = [("linear", True), ("nearest", True), ("linear", False), ("nearest", False)]      # (filter, chain + mipmap filter)
OFFSETS = [(0, 0), (1, 0), (-3, 2), (7, -8), (9, 0)]                  # the last beyond every extent here but 16
PROBE_UNIFORMS = [("sampler2D", "tex"), ("sampler2D", "operands"), ("sampler2D", "gradients"), ("int", "form")]


@dataclass(frozen=True)
class Config:
    """one sampled texture (configs() says which ones there are)"""
    width: int
    height: int
    format: str
    filter: str
    chain: bool
    repeat_x: bool
    repeat_y: bool

    @property
    def name(self) -> str:
        return (f"{self.width}x{self.height}.{self.format}.{self.filter}{'.chain' if self.chain else ''}."
                f"{'repeat' if self.repeat_x else 'clamp'}-{'repeat' if self.repeat_y else 'clamp'}")

    @property
    def data(self) -> np.ndarray:
        return _data(self.width, self.height, self.format)

    @property
    def top(self) -> int:
        return (max(self.width, self.height).bit_length() - 1) if self.chain else 0


@lru_cache(maxsize=None)
def _data(width: int, height: int, format: str) -> np.ndarray:
    dtype, components = FORMATS[format]
    rng = np.random.default_rng(width*1000 + height*10 + components)
    if dtype == np.uint8:
        data = rng.integers(0, 256, (height, width, components)).astype(np.uint8)
    else:
        data = rng.random((height, width, components)).astype(dtype)
    data.setflags(write=False)
    return data


def configs() -> list[Config]:
    """NOT the full product size x format x wrap x mode (256 textures, each with some 40 forms over 84 to 210 rows — minutes of exact
    arithmetic): a Latin square of 16, in which every size meets every format, every wrap pair and every mode once, and every (wrap
    pair, mode) combination occurs once; plus the combinations a square of 16 cannot hold and a kernel can get wrong on their own —
    the trilinear blend over RGB8 levels (the unaligned 32-bit load at a level's last texel, reached through the FILTER) on 8x8 and
    on the odd 5x3, over RGBA8 on 5x3 and 16x4, and the nearest-level rule on RGB8 5x3."""
    out = []
    for si, (w, h) in enumerate(SIZES):
        for fi, format in enumerate(FORMATS):
            (filter, chain), (rx, ry) = MODES[(fi + si) % 4], WRAPS[(fi + 2*si + 1) % 4]
            out.append(Config(w, h, format, filter, chain, rx, ry))
    out += [Config(8, 8, "rgb8", "linear", True, True, True), Config(5, 3, "rgb8", "linear", True, False, False),
            Config(5, 3, "rgba8", "linear", True, True, False), Config(16, 4, "rgba8", "linear", True, False, True),
            Config(5, 3, "rgb8", "nearest", True, True, True),
            Config(16, 4, "r32f", "linear", False, True, True)]              # (a third texture for the roll identity)
    return out


CONFIGS = configs()


@lru_cache(maxsize=None)
def oracle_texture(config: Config) -> O.Texture:
    texture = O.make_texture(config.data, config.filter, config.repeat_x, config.repeat_y)
    return O.build_mipmaps(texture) if config.chain else texture


@lru_cache(maxsize=None)
def reference(config: Config) -> R.Texture:
    """the restatement's texture: level 0 and, with a chain, the oracle's levels (what both builds sample: the host build is handed
    the oracle's chain, tests/test_gpu_mip.py holds the device's chain kernel to the same bytes)"""
    texture = oracle_texture(config)
    levels = [config.data] + ([O.mip_level(texture, k) for k in range(1, texture.levels)] if config.chain else [])
    return R.Texture(levels, config.filter, config.chain, config.repeat_x, config.repeat_y)


# ---- operands ---------------------------------------------------------------------------------------------------------------------

def coordinates(width: int, height: int) -> np.ndarray:
    """texel centres, texel edges, one texel outside on either side and a seeded handful in between: (n, 2) float32"""
    w, h = float(width), float(height)
    fixed = [(0.5/w, 0.5/h), ((w - 0.5)/w, (h - 0.5)/h), (0.0, 0.0), (1.0, 1.0), (1.0/w, 0.0) if width > 1 else (0.5, 0.5),
             (-1.0/w, -1.0/h), ((w + 1.0)/w, (h + 1.0)/h), (-0.5/w, (h + 0.5)/h)]
    rng = np.random.default_rng(width*31 + height)
    return np.concatenate([np.array(fixed, np.float64), rng.uniform(-0.4, 1.4, (4, 2))]).astype(F)


def lods(top: int) -> list[float]:
    return [-1.0, 0.0, 0.5, 1.0, 1.25, float(top), float(top + 3)]


def sample_rows(width: int, height: int, top: int) -> np.ndarray:
    """(rows, 8) float32: uv, lod, q | dPdx, dPdy — every coordinate at every lod; the gradients are ones whose lambda is the row's
    lod on a power-of-two extent (2^lod texels along x, half that along y), with a diagonal pair on every third row"""
    rows = []
    for k, uv in enumerate(coordinates(width, height)):
        for n, lod in enumerate(lods(top)):
            reach = 2.0**lod
            if (k + n) % 3 == 2:
                dpdx, dpdy = (0.6*reach/width, 0.8*reach/height), (-0.4*reach/width, 0.3*reach/height)
            else:
                dpdx, dpdy = (reach/width, 0.0), (0.0, 0.5*reach/height)
            rows.append([uv[0], uv[1], lod, [0.5, 2.0, -3.0, 1.0][(k + n) % 4], *dpdx, *dpdy])
    assert len(rows) <= ROWS
    return np.array(rows, np.float64).astype(F)


def fetch_rows(width: int, height: int, top: int) -> np.ndarray:
    """(rows, 8): texel coordinates from -1 to one past the extent of level 0 — inside and outside of every level — at every lod
    from -1 to top + 1, as floats"""
    xs = sorted({-1, 0, 1, width//2, width - 1, width})
    ys = sorted({-1, 0, height//2, height - 1, height})
    rows = [[x, y, lod, 0, 0, 0, 0, 0] for lod in range(-1, top + 2) for x in xs for y in ys][:ROWS]
    return np.array(rows, F)


def operand_textures(rows: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """the two (16, 16, 4) operand textures of a row table; unused rows read zeros"""
    padded = np.zeros((ROWS, 8), F)
    padded[:len(rows)] = rows
    return (np.ascontiguousarray(padded[:, :4].reshape(HEIGHT, WIDTH, 4)), np.ascontiguousarray(padded[:, 4:].reshape(HEIGHT, WIDTH, 4)))


# ---- probes -----------------------------------------------------------------------------------------------------------------------

def _ivec(offset) -> str:
    return f"ivec2({offset[0]}, {offset[1]})"


PROLOGUE = """
    ivec2 at = ivec2(gl_FragCoord.xy);
    vec4 a = texelFetch(operands, at, 0);
    vec4 g = texelFetch(gradients, at, 0);
    vec2 uv = a.xy; float lod = a.z; float q = a.w;
    vec4 c = vec4(-1.0);
"""

# form name -> GLSL expression; "name@k" is the form with OFFSETS[k]
EXPLICIT_FORMS: dict[str, str] = {"echo": "a", "echo.gradients": "g", "texture": "texture(tex, uv)", "textureLod": "textureLod(tex, uv, lod)",
                                  "textureGrad": "textureGrad(tex, uv, g.xy, g.zw)", "texelFetch": "texelFetch(tex, ivec2(a.xy), int(lod))",
                                  "textureSize": "vec4(vec2(textureSize(tex, int(lod))), 0.0, 0.0)"}
for _k, _o in enumerate(OFFSETS):
    EXPLICIT_FORMS[f"textureOffset@{_k}"] = f"textureOffset(tex, uv, {_ivec(_o)})"
    EXPLICIT_FORMS[f"textureLodOffset@{_k}"] = f"textureLodOffset(tex, uv, lod, {_ivec(_o)})"
    EXPLICIT_FORMS[f"textureGradOffset@{_k}"] = f"textureGradOffset(tex, uv, g.xy, g.zw, {_ivec(_o)})"
    EXPLICIT_FORMS[f"texelFetchOffset@{_k}"] = f"texelFetchOffset(tex, ivec2(a.xy), int(lod), {_ivec(_o)})"

PROJ_OFFSET = 2                                                       # the projective forms take OFFSETS[2]
PROJ_FORMS: dict[str, str] = {}
for _n, _p in (("3", "vec3(uv, q)"), ("4", "vec4(uv, 7.0, q)")):
    PROJ_FORMS.update({
        f"textureProj{_n}": f"textureProj(tex, {_p})", f"textureProjLod{_n}": f"textureProjLod(tex, {_p}, lod)",
        f"textureProjOffset{_n}": f"textureProjOffset(tex, {_p}, {_ivec(OFFSETS[PROJ_OFFSET])})",
        f"textureProjLodOffset{_n}": f"textureProjLodOffset(tex, {_p}, lod, {_ivec(OFFSETS[PROJ_OFFSET])})",
        f"textureProjGrad{_n}": f"textureProjGrad(tex, {_p}, g.xy, g.zw)",
        f"textureProjGradOffset{_n}": f"textureProjGradOffset(tex, {_p}, g.xy, g.zw, {_ivec(OFFSETS[PROJ_OFFSET])})"})
# the form a projective one must equal once it is fed the divided coordinate
PROJ_TWIN = {"textureProj": "texture", "textureProjLod": "textureLod", "textureProjOffset": f"textureOffset@{PROJ_OFFSET}",
             "textureProjLodOffset": f"textureLodOffset@{PROJ_OFFSET}", "textureProjGrad": "textureGrad",
             "textureProjGradOffset": f"textureGradOffset@{PROJ_OFFSET}"}


def probe_glsl(forms: dict[str, str]) -> str:
    branches = "\n".join(f"    {'if' if k == 0 else 'else if'} (form == {k}) c = {expression};" for k, expression in enumerate(forms.values()))
    return "void main() {" + PROLOGUE + branches + "\n    fragColor = c;\n}\n"


def form_index(forms: dict[str, str], name: str) -> int:
    return list(forms).index(name)


# a box blur of (2*BLUR_REACH + 1)^2 textureOffset taps in a loop: the fragment the LDS tile is for
BLUR_REACH = 1
BLUR_GLSL = f"""
void main() {{
    vec4 sum = vec4(0.0);
    for (int x = -{BLUR_REACH}; x <= {BLUR_REACH}; x++)
        for (int y = -{BLUR_REACH}; y <= {BLUR_REACH}; y++)
            sum += textureOffset(tex, astuv*1.25 - 0.125, ivec2(x, y));
    fragColor = sum/{float((2*BLUR_REACH + 1)**2)!r};
}}
"""

# bias and implicit derivatives (device only: the host build has no quad). uv is the pixel position rotated and scaled so that
# lambda_base runs from magnification to beyond the top level across the target: the footprint grows with the pixel's index.
# x: texture(s, uv) against textureGrad with the quad's differences; y, z, w: texture(s, uv, b) against textureLod(s, uv,
# lambda_base + b), lambda_base restated with the same log2. A component is 0 where the two agree bit for bit in all four channels.
BIAS_VALUES = [-1.0, 0.5, 2.0]
BIAS_GLSL = """
float same(vec4 p, vec4 r) { return (floatBitsToInt(p) == floatBitsToInt(r)) ? 0.0 : 1.0; }
void main() {
    vec2 p = gl_FragCoord.xy - 0.5;
    float k = p.y*16.0 + p.x;
    float scale = exp2(k/32.0 - 2.5)/16.0;
    vec2 uv = scale*vec2(0.8*p.x - 0.6*p.y, 0.6*p.x + 0.8*p.y) + 0.3;
    if (form == 1) { fragColor = vec4(uv, 0.0, 0.0); return; }
    vec2 t = uv*vec2(textureSize(tex, 0));
    float dudx = dFdx(t.x), dvdx = dFdx(t.y), dudy = dFdy(t.x), dvdy = dFdy(t.y);
    float along_x = dudx*dudx + dvdx*dvdx, along_y = dudy*dudy + dvdy*dvdy;
    float base = 0.5*log2(along_x > along_y ? along_x : along_y);
    if (form == 2) { fragColor = vec4(base, dudx, dvdx, dudy); return; }
    fragColor = vec4(same(texture(tex, uv), textureGrad(tex, uv, dFdx(uv), dFdy(uv))),
                     same(texture(tex, uv, -1.0), textureLod(tex, uv, base + -1.0)),
                     same(texture(tex, uv, 0.5), textureLod(tex, uv, base + 0.5)),
                     same(texture(tex, uv, 2.0), textureLod(tex, uv, base + 2.0)));
}
"""



def bias_uv() -> np.ndarray:
    """BIAS_GLSL's uv restated in numpy float32, one rounding per operation as the fragment has them (exp2 is the oracle's
    restatement of sfmath's): (HEIGHT, WIDTH, 2), [y, x]"""
    x, y = np.meshgrid(np.arange(WIDTH, dtype=F), np.arange(HEIGHT, dtype=F))
    k = y*F(16.0) + x
    scale = O.math("exp2", k/F(32.0) - F(2.5)).astype(F)/F(16.0)
    u = scale*(F(0.8)*x - F(0.6)*y) + F(0.3)
    v = scale*(F(0.6)*x + F(0.8)*y) + F(0.3)
    return np.stack([u, v], axis=-1).astype(F)


def quad_lambda(uv: np.ndarray, size: tuple) -> np.ndarray:
    """lambda_base of every pixel of a frame of coordinates (h, w, 2) by the restatement: the differences of uv*(width, height) across
    the pixel's 2 x 2 quad, the "fine" form (each row and column of the quad has its own)"""
    t = (uv*np.array(size, F)).astype(F)
    h, w = uv.shape[:2]
    x0, y0 = (np.arange(w) & ~1), (np.arange(h) & ~1)
    ddx, ddy = t[:, x0 + 1] - t[:, x0], t[y0 + 1] - t[y0]
    base = R.Texture([np.zeros((1, 1, 1), F)], "linear", False, True, True).lambda_base
    return np.array([[base(float(ddx[j, i, 0]), float(ddx[j, i, 1]), float(ddy[j, i, 0]), float(ddy[j, i, 1])) for i in range(w)] for j in range(h)], F)


def covers_every_level(lam: np.ndarray, top: int) -> bool:
    """a pixel in lambda <= 0, in each interval (d, d + 1) and above the top level"""
    return bool((lam <= 0).any() and (lam > top).any() and all(((lam > d) & (lam < d + 1)).any() for d in range(top)))


# ---- expected values --------------------------------------------------------------------------------------------------------------

def expected(config: Config, name: str, rows: np.ndarray) -> np.ndarray:
    """(len(rows), 4) float32 by the restatement, for the non-projective forms"""
    texture = reference(config)
    function, _, k = name.partition("@")
    offset = OFFSETS[int(k)] if k else (0, 0)
    out = np.zeros((len(rows), 4), F)
    for n, row in enumerate(rows):
        uv, lod, dpdx, dpdy = (float(row[0]), float(row[1])), float(row[2]), (float(row[4]), float(row[5])), (float(row[6]), float(row[7]))
        if function in ("texture", "textureOffset"):
            out[n] = texture.at_level(0, uv, offset)                 # on the host build: no quad, level 0
        elif function in ("textureLod", "textureLodOffset"):
            out[n] = texture.at_lambda(uv, lod, offset)
        elif function in ("textureGrad", "textureGradOffset"):
            out[n] = texture.grad(uv, dpdx, dpdy, offset)
        elif function in ("texelFetch", "texelFetchOffset"):
            out[n] = texture.fetch((int(row[0]) + offset[0], int(row[1]) + offset[1]), int(lod))
        elif function == "textureSize":
            out[n] = (*texture.size(int(lod)), 0.0, 0.0)
        else:
            raise KeyError(name)
    return out


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same_bits(got: np.ndarray, want: np.ndarray, what) -> None:
    differ = np.flatnonzero((bits(got) != bits(want)).reshape(len(got), -1).any(axis=1))
    assert differ.size == 0, (what, f"{differ.size}/{len(got)} rows differ; first: row {differ[0]} got {got[differ[0]]} want {want[differ[0]]}")


# ---- evaluation -------------------------------------------------------------------------------------------------------------------
# `run(probe, config, form, operands, gradients) -> (ROWS, 4) float32` renders one form of a probe ("explicit" / "proj") over one row
# table with `config`'s texture bound; the host and the device test each supply theirs.

def rows_of(config: Config, name: str) -> np.ndarray:
    table = fetch_rows if name.startswith(("texelFetch", "textureSize")) else sample_rows
    return table(config.width, config.height, config.top)


def implicit(config: Config, name: str) -> bool:
    """the form takes its level of detail from the quad's differences on this texture (the host build has no quad: level 0)"""
    return config.chain and name.partition("@")[0].rstrip("34") in ("texture", "textureOffset", "textureProj", "textureProjOffset")


def evaluate(run, probe: str, forms: dict[str, str]) -> dict:
    """{(config, form name): (rows, 4)} for every config and every form of the probe"""
    out = {}
    for config in CONFIGS:
        for k, name in enumerate(forms):
            rows = rows_of(config, name)
            out[config, name] = run(probe, config, k, *operand_textures(rows))[:len(rows)]
    return out


def check_echo(results: dict) -> None:
    for config in CONFIGS:
        rows = rows_of(config, "echo")
        assert_same_bits(results[config, "echo"], rows[:, :4], (config.name, "echo"))
        assert_same_bits(results[config, "echo.gradients"], rows[:, 4:], (config.name, "echo.gradients"))


def check_reference(results: dict, skip_implicit: bool = False) -> None:
    """every non-projective form against the restatement, bit for bit"""
    for (config, name), got in results.items():
        if name.startswith("echo") or (skip_implicit and implicit(config, name)):
            continue
        assert_same_bits(got, expected(config, name, rows_of(config, name)), (config.name, name))


def check_projective(run, explicit: dict, proj: dict, skip_implicit: bool = False) -> None:
    """every textureProj* form equals its twin fed the divided coordinate (binary32 division, correctly rounded as numpy's is)"""
    twin_forms = list(EXPLICIT_FORMS)
    for (config, name), got in proj.items():
        if skip_implicit and implicit(config, name):
            continue
        rows = rows_of(config, name).copy()
        rows[:, 0], rows[:, 1] = rows[:, 0]/rows[:, 3], rows[:, 1]/rows[:, 3]
        twin = PROJ_TWIN[name[:-1]]
        want = run("explicit", config, twin_forms.index(twin), *operand_textures(rows))[:len(rows)]
        assert_same_bits(got, want, (config.name, name, "against", twin))


def check_identities(run, explicit: dict) -> None:
    forms = list(EXPLICIT_FORMS)
    for config in CONFIGS:
        rows = rows_of(config, "texture")
        if not config.chain:                                          # without a chain a lod selects nothing
            assert_same_bits(explicit[config, "textureLod"], explicit[config, "texture"], (config.name, "textureLod without a chain"))
            assert_same_bits(explicit[config, "textureGrad"], explicit[config, "texture"], (config.name, "textureGrad without a chain"))
            if config.repeat_x and config.repeat_y:                   # an offset is a roll of the array
                for k, (dx, dy) in enumerate(OFFSETS):
                    data = np.roll(config.data, (-dy, -dx), axis=(0, 1))
                    want = run("explicit", config, forms.index("texture"), *operand_textures(rows), data=data)[:len(rows)]
                    assert_same_bits(explicit[config, f"textureOffset@{k}"], want, (config.name, "textureOffset as a roll", (dx, dy)))
