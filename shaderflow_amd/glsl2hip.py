"""
glsl2hip — fragments that are not in the kernel registry: GLSL 3.30 → HIP C++ → gfx950 code object.

The reference gives the assembled GLSL to the OpenGL driver (shader.py:190-239 builds the text, :313-349 compiles it
with `opengl.program`, falling back to `missing.glsl` on errors). Without a driver the same job is done in two steps:

1. `translate()` rewrites the fragment token by token into the body of a C++ struct that derives from
   `sf::rt::FragmentBase` (csrc/jit_runtime.hpp): globals and uniforms become members, functions become member
   functions, `main` becomes `main_`. GLSL and C++ share almost all of their expression and statement syntax; the
   header supplies the vector types (with swizzles), the built-in functions on the deterministic binary32 routines of
   csrc/sfmath.hpp, the whole sampler2D column of the §8.7 texture lookups (explicit lod, bias, gradients, offsets, projection,
   fetches of any level: csrc/glsl.hpp "THE RULES") and the reference's prelude, so what is rewritten is small:
     * floating literals get an `f` suffix (C++ would compute in double),
     * `in/out/inout` parameter qualifiers become values and references, precision/layout/interpolation qualifiers go,
     * `uniform`/`in`/`out` declarations go (the members exist already), prototypes go,
     * `int(x)`/`uint(x)` become `to_int(x)`/`to_uint(x)` (defined results for NaN and overflow),
     * arrays are values in GLSL (§4.1.9, §5.8-5.9) and become the header's `sf_arr<T,n>`: `T name[n]`, `T[n] name`, `T[n] a, b`
       and `T w[] = T[](…)` as locals, globals, members, parameters (an `in` array is the callee's copy) and return types; the
       constructor `T[n](a, b)` becomes `sf_arr_of<T>(a, b)`; `x.length()` of any postfix expression becomes `length_of(x)`,
     * a struct gets `bool operator==(const S&) const = default;` (§5.9: member by member),
     * a swizzle passed for an `out`/`inout` parameter of one of the fragment's functions (or of `modf`) goes through `sf_out(…)`,
       which hands the function a vector and writes it back through the swizzle after the call,
     * `const` scalars with literal initialisers become `static constexpr` (array bounds),
     * `discard` sets a flag and returns, identifiers that are C++ keywords get a trailing underscore,
     * a `#define` continued with backslash-newline is spliced; `#line` before every function body (and after a directive inside
       one) keeps `__LINE__` and the compiler's messages on the lines of the GLSL text.
2. `compile()` runs hipcc (`--genco`, the flags of csrc/Makefile) and caches the code object by content hash;
   libshaderflow_hip loads it with `sfx_program_load`.

The rule (tests/language_cases.py holds it row by row): a fragment that is valid GLSL 3.30 computes GLSL's value, or
`translate()` refuses it by name with a `TranslationError` (the caller logs it and binds the `missing` kernel, like the reference
does for a GLSL compile error) — nothing is left to fail inside hipcc seconds later. Refused:
     * `&&` next to `^^` without parentheses (`^^` is written `!=`, which binds tighter than `&&`),
     * a C++ keyword used as an identifier together with its renamed form (`new` and `new_`),
     * an array without a size whose initialiser is not an array constructor (`float b[] = a;`),
     * non-square matrices and samplers other than `sampler2D` (the types do not exist here),
     * uniforms of other types than scalars, vectors, square matrices and `sampler2D`, uniform arrays of more than one dimension or
       with a size that is no literal or literal `const int`, uniform initialisers that are no literal constant expressions, more
       than 16 samplers or 64 uniform floats.
Known limits that are not refused: there is no geometry beyond one fullscreen quad; `out`/`inout` parameters are references, so a
function that writes one and then reads the same variable under its global name sees its own write, where GLSL copies out on
return; `%` of a negative operand, undefined in GLSL, is C's.
"""
from __future__ import annotations

import hashlib
import os
import re
import subprocess
from dataclasses import dataclass, field
from pathlib import Path
from typing import Iterable, Optional

CSRC = Path(__file__).resolve().parent/"csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++20", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math",
         "-fno-slp-vectorize", "-fno-gpu-flush-denormals-to-zero", "-fwrapv",      # GLSL integers wrap (§4.1.3); C++ leaves signed overflow undefined
         "-Wno-unused-value", "-Wno-deprecated-copy", "-Wno-parentheses"]

USER_SLOTS = 64          # csrc/glsl.hpp USER_SLOTS
TEX_SLOTS = 16           # csrc/glsl.hpp TEX_SLOTS
FIXED_SAMPLER_SLOTS = {"iSpectrogram": 1, "iWaveform": 2}      # the slots the tape patches per frame (render_kernels.hpp frame_view)
AUDIO_UNIFORMS = {"iAudioVolume", "iAudioVolumeIntegral", "iAudioSTD", "iSpectrogramOffset"}   # … and the uniforms it patches (sfx_jit_flags bit 1)


class TranslationError(Exception):
    pass


class CompileError(Exception):
    pass


@dataclass
class Binding:
    """One name the host sets on the program: a uniform (`slot` = first float of csrc Uniforms.user) or a sampler (`slot` = texture slot)"""
    name: str
    type: str
    slot: int
    count: int = 1
    integer: bool = False
    default: Optional[tuple] = None      # the initialiser of `uniform T name = …;` (GLSL 3.30 §4.3.5): what the program reads until the host sets the uniform
    array: Optional[str] = None          # element `name[i]` of the uniform array `array` (GL exposes array elements under these names too)

    @property
    def sampler(self) -> bool:
        return self.type == "sampler2D"


@dataclass
class Translation:
    cpp: str
    bindings: list[Binding] = field(default_factory=list)
    tiled_sampler: Optional[str] = None            # the sampler the kernels serve from an LDS tile (jit_runtime.hpp TileView), if any

    @property
    def key(self) -> str:
        return hashlib.sha256((self.cpp + runtime_fingerprint()).encode()).hexdigest()[:24]


# ---- tokens -----------------------------------------------------------------------------------------------------------

_TOKEN = re.compile(r"""
    (?P<comment>//[^\n]*|/\*.*?\*/)
  | (?P<pp>\#(?:[^\n\\]|\\.|\\\n)*)
  | (?P<number>0[xX][0-9a-fA-F]+[uU]?|(?:\d+\.\d*|\.\d+|\d+)(?:[eE][+-]?\d+)?(?:lf|LF|[fFuU])?)
  | (?P<ident>[A-Za-z_]\w*)
  | (?P<op><<=|>>=|\+\+|--|<<|>>|<=|>=|==|!=|&&|\|\||\^\^|[-+*/%&|^]=|[-+*/%<>=!&|^~?:;,.(){}\[\]])
  | (?P<ws>\s+)
""", re.X | re.S)

_CPP_ONLY_KEYWORDS = {
    "new", "delete", "operator", "private", "protected", "friend", "virtual", "explicit", "mutable", "try", "catch", "throw",
    "typename", "auto", "register", "signed", "char", "wchar_t", "char8_t", "char16_t", "char32_t", "and", "or", "not", "xor", "bitand",
    "bitor", "compl", "and_eq", "or_eq", "xor_eq", "not_eq", "nullptr", "constexpr", "consteval", "constinit", "decltype", "noexcept",
    "static_assert", "thread_local", "alignas", "alignof", "concept", "requires", "co_await", "co_return", "co_yield", "export",
    "import", "module", "final", "override", "asm", "typeid", "dynamic_cast", "static_cast", "reinterpret_cast", "const_cast",
}
_DROPPED_QUALIFIERS = {"highp", "mediump", "lowp", "flat", "smooth", "noperspective", "centroid", "invariant", "precise"}
_TYPES = {"void", "float", "int", "uint", "bool", "vec2", "vec3", "vec4", "ivec2", "ivec3", "ivec4", "uvec2", "uvec3", "uvec4",
          "bvec2", "bvec3", "bvec4", "mat2", "mat3", "mat4", "mat2x2", "mat3x3", "mat4x4", "sampler2D"}
_UNIFORM_COUNTS = {"float": (1, False), "int": (1, True), "bool": (1, True), "uint": (1, True), "vec2": (2, False), "vec3": (3, False),
                   "vec4": (4, False), "ivec2": (2, True), "ivec3": (3, True), "ivec4": (4, True),
                   "uvec2": (2, True), "uvec3": (3, True), "uvec4": (4, True),
                   "mat2": (4, False), "mat3": (9, False), "mat4": (16, False)}
# members of sf::rt::FragmentBase (jit_runtime.hpp): uniforms and varyings that exist for every fragment
BUILTIN_MEMBERS = {
    "fragCoord", "stxy", "glxy", "stuv", "astuv", "gluv", "agluv", "gl_FragCoord", "fragColor", "instance",
    "iTime", "iTau", "iDuration", "iFrametime", "iDeltatime", "iCycle", "iAspectRatio", "iWidth", "iHeight", "iResolution", "iMouse",
    "iWantAspect", "iQuality", "iSSAA", "iFramerate", "iFrame", "iLayer", "iSubsample", "iRealtime", "iRendering", "iMouseInside",
    "iMouse1", "iMouse2", "iCameraMode", "iCameraProjection", "iCameraRight", "iCameraUpward", "iCameraForward", "iCameraPosition",
    "iCameraZenith", "iCameraSeparation", "iCameraZoom", "iCameraIsometric", "iCameraFocalLength", "iCameraOrbital", "iCameraDolly",
    "iAudioVolume", "iAudioVolumeIntegral", "iAudioSTD", "iSpectrogramLength", "iSpectrogramBins", "iSpectrogramScroll",
    "iWaveformLength", "iSpectrogramSmooth", "iSpectrogramOffset", "iSpectrogramMin", "iSpectrogramMax",
}


@dataclass
class Tok:
    kind: str
    text: str


def tokenize(source: str) -> list[Tok]:
    tokens, position = [], 0
    while position < len(source):
        match = _TOKEN.match(source, position)
        if match is None or (match.lastgroup == "pp" and source[source.rfind("\n", 0, position) + 1:position].strip()):
            raise TranslationError(f"unexpected character {source[position]!r} at offset {position}")
        tokens.append(Tok(match.lastgroup, match.group()))
        position = match.end()
    return tokens


def _float_literal(text: str) -> str:
    if text[:2] in ("0x", "0X") or text[-1] in "uU":
        return text
    if text.endswith(("lf", "LF")):
        text = text[:-2]
    if text[-1] in "fF":
        return text
    if ("." in text) or ("e" in text) or ("E" in text):
        return text + ("f" if "." in text or "e" in text.lower() else "")
    return text


def _matching(tokens: list[Tok], start: int, open_: str, close: str) -> int:
    """index of the token closing the bracket opened at `start`"""
    depth = 0
    for k in range(start, len(tokens)):
        if tokens[k].kind == "op":
            if tokens[k].text == open_:
                depth += 1
            elif tokens[k].text == close:
                depth -= 1
                if depth == 0:
                    return k
    raise TranslationError(f"unbalanced {open_!r}")


def _significant(tokens: list[Tok], start: int, step: int = 1) -> int:
    """next index from `start` (inclusive) in direction `step` that is not whitespace or a comment; len(tokens) / -1 if none"""
    k = start
    while 0 <= k < len(tokens) and tokens[k].kind in ("ws", "comment"):
        k += step
    return k


# ---- token-level rewrites that apply everywhere --------------------------------------------------------------------------

def _is_length_call(tokens: list[Tok], dot: int) -> bool:
    name = _significant(tokens, dot + 1)
    if name >= len(tokens) or tokens[name].text != "length":
        return False
    open_ = _significant(tokens, name + 1)
    close = _significant(tokens, open_ + 1) if open_ < len(tokens) else len(tokens)
    return open_ < len(tokens) and tokens[open_].text == "(" and close < len(tokens) and tokens[close].text == ")"


_QUALIFIERS = {"in", "out", "inout", "const"} | _DROPPED_QUALIFIERS
_SWIZZLE = re.compile(r"[xyzw]{2,4}|[rgba]{2,4}|[stpq]{2,4}")
_BUILTIN_OUT_PARAMETERS = {"modf": {1}}
_STATEMENT_WORDS = {"return", "if", "else", "while", "for", "do", "switch", "case"}


def _split_top_level(tokens: list[Tok]) -> list[list[Tok]]:
    """the token runs between the commas that are inside no bracket"""
    parts, depth, current = [], 0, []
    for t in tokens:
        if t.kind == "op" and t.text in ("(", "[", "{"):
            depth += 1
        elif t.kind == "op" and t.text in (")", "]", "}"):
            depth -= 1
        if t.kind == "op" and t.text == "," and depth == 0:
            parts.append(current); current = []
        else:
            current.append(t)
    if any(t.kind not in ("ws", "comment") for t in current):
        parts.append(current)
    return parts


def _postfix_start(out: list[Tok]) -> int:
    """index in `out` where the postfix expression that ends `out` begins: `s.w`, `a[1].b`, `f(x)[2]`, `name`"""
    k = len(out)
    while True:
        j = _significant(out, k - 1, -1)
        if j < 0:
            return k
        t = out[j]
        if t.kind == "op" and t.text in (")", "]"):
            depth = 0
            while j >= 0:
                if out[j].kind == "op" and out[j].text in (")", "]"):
                    depth += 1
                elif out[j].kind == "op" and out[j].text in ("(", "["):
                    depth -= 1
                    if depth == 0:
                        break
                j -= 1
            if j < 0:
                raise TranslationError("unbalanced bracket before .length()")
            k = j
        elif t.kind == "ident" and t.text not in _STATEMENT_WORDS:
            k = j
            dot = _significant(out, j - 1, -1)
            if dot >= 0 and out[dot].kind == "op" and out[dot].text == ".":
                k = dot
                continue
            return k
        else:
            return k


def out_parameters(tokens: list[Tok], types: set[str]) -> dict[str, set[int]]:
    """function name → positions of its `out` / `inout` parameters (every overload of a name together), the built-ins' included"""
    found = {name: set(positions) for name, positions in _BUILTIN_OUT_PARAMETERS.items()}
    depth = 0
    for k, t in enumerate(tokens):
        if t.kind == "op" and t.text in "{}":
            depth += 1 if t.text == "{" else -1
        elif depth == 0 and t.kind == "ident" and t.text in types:
            name = _significant(tokens, k + 1)
            if name < len(tokens) and tokens[name].kind == "op" and tokens[name].text == "[":
                name = _significant(tokens, _matching(tokens, name, "[", "]") + 1)
            open_ = _significant(tokens, name + 1)
            if open_ < len(tokens) and tokens[name].kind == "ident" and tokens[open_].kind == "op" and tokens[open_].text == "(":
                parameters = _split_top_level(tokens[open_ + 1:_matching(tokens, open_, "(", ")")])
                positions = {i for i, p in enumerate(parameters) if any(w.kind == "ident" and w.text in ("out", "inout") for w in p)}
                if positions:
                    found.setdefault(tokens[name].text, set()).update(positions)
    return found


def _is_swizzle(tokens: list[Tok]) -> bool:
    """the expression ends in a swizzle of two to four components (`v.zw`, `m[1].yx`)"""
    last = _significant(tokens, len(tokens) - 1, -1)
    dot = _significant(tokens, last - 1, -1) if last > 0 else -1
    return dot >= 0 and tokens[last].kind == "ident" and bool(_SWIZZLE.fullmatch(tokens[last].text)) and tokens[dot].kind == "op" and tokens[dot].text == "."


def _declarators(tokens: list[Tok], start: int, types: set[str]) -> tuple[list, int]:
    """the declarators from the name at tokens[start]: [(name, tokens of `[size]` or None, tokens of the initialiser or None)] and
    the index of the token that ends them (`;`, `)`, the comma before the next parameter, `(` of a function head)"""
    found = []
    k = start
    while True:
        j = _significant(tokens, k + 1)
        size = initialiser = None
        if j < len(tokens) and tokens[j].kind == "op" and tokens[j].text == "[":
            close = _matching(tokens, j, "[", "]")
            size = tokens[j + 1:close]
            j = _significant(tokens, close + 1)
        if j < len(tokens) and tokens[j].kind == "op" and tokens[j].text == "=":
            depth, end = 0, j + 1
            while end < len(tokens):
                text = tokens[end].text if tokens[end].kind == "op" else ""
                if text in ("(", "[", "{"):
                    depth += 1
                elif text in (")", "]", "}"):
                    if depth == 0:
                        break
                    depth -= 1
                elif depth == 0 and text in (",", ";"):
                    break
                end += 1
            initialiser = tokens[j + 1:end]
            j = end
        found.append((tokens[k], size, initialiser))
        if j < len(tokens) and tokens[j].kind == "op" and tokens[j].text == ",":
            name = _significant(tokens, j + 1)
            after = _significant(tokens, name + 1)
            if (after < len(tokens) and tokens[name].kind == "ident" and tokens[name].text not in types | _QUALIFIERS
                    and tokens[after].kind == "op" and tokens[after].text in ("[", "=", ",", ";")):
                k = name
                continue
        return found, j


def _constructor_length(name: str, initialiser: Optional[list[Tok]]) -> str:
    """the size of `T name[] = T[n](…)` or `= T[](a, b, c)`"""
    words = [t for t in (initialiser or []) if t.kind not in ("ws", "comment")]
    if len(words) > 3 and words[1].text == "[":
        close = _matching(words, 1, "[", "]")
        if close + 1 < len(words) and words[close + 1].text == "(":
            if close > 2:
                return "".join(t.text for t in words[2:close])
            return str(len(_split_top_level(words[close + 2:_matching(words, close + 1, "(", ")")])))
    raise TranslationError(f"array '{name}' is declared without a size: its initialiser must be an array constructor")


def _array_declaration(tokens: list[Tok], k: int, types: set[str], structs: set[str], outs: dict, out: list[Tok]) -> Optional[int]:
    """`T a[3], b`, `T[2] p, q`, `T w[] = T[](…)`, `T[2] f(` at tokens[k] == T → `sf_arr<T,3> a; T b`, `sf_arr<T,2> p, q`, … appended to
    `out`; returns the index of the last token it took, or None when no array is declared there (the text then stays as it is)"""
    nxt = _significant(tokens, k + 1)
    prefix = None
    first = nxt
    if tokens[nxt].kind == "op":
        close = _matching(tokens, nxt, "[", "]")
        first = _significant(tokens, close + 1)
        prefix = tokens[nxt + 1:close]
    if first >= len(tokens) or tokens[first].kind != "ident":
        return None
    found, end = _declarators(tokens, first, types)
    if prefix is None and all(size is None for (_, size, _) in found):
        return None
    before = _significant(out, len(out) - 1, -1)
    constant = "const " if before >= 0 and out[before].kind == "ident" and out[before].text == "const" else ""
    emitted: list[Tok] = []
    previous = None
    for (name, size, initialiser) in found:
        bound = size if size is not None else prefix
        type_ = tokens[k].text
        if bound is not None:
            length = re.sub(r"\s+", "", _text(_rewrite_tokens(bound, structs, outs))) or _constructor_length(name.text, initialiser)
            type_ = f"sf_arr<{type_},{length}>"
        declared = _text(_rewrite_tokens([name], structs, outs))
        if previous is not None:                                   # one C++ declaration cannot mix `sf_arr<T,3> a` with `T b`
            emitted.append(Tok("op", ", " if type_ == previous else f"; {constant}"))
        if type_ != previous:
            emitted += [Tok("ident", type_), Tok("ws", " ")]
        emitted.append(Tok("ident", declared))
        if initialiser is not None:
            emitted += [Tok("ws", " "), Tok("op", "=")] + _rewrite_tokens(initialiser, structs, outs)
        previous = type_
    dropped = _text(tokens[k:end]).count("\n") - _text(emitted).count("\n")      # keep the line count of the source
    out.extend(emitted)
    if dropped > 0:
        out.append(Tok("ws", "\n"*dropped))
    return end - 1


def _rewrite_tokens(tokens: list[Tok], structs: set[str], outs: Optional[dict] = None, uniform: bool = False) -> list[Tok]:
    out: list[Tok] = []
    k = 0
    types = _TYPES | structs
    outs = outs or {}
    while k < len(tokens):
        t = tokens[k]
        if t.kind == "op" and t.text == ";":
            uniform = False
        if t.kind == "comment":
            out.append(Tok("ws", "\n"*t.text.count("\n") or " "))
        elif t.kind == "number":
            out.append(Tok("number", _float_literal(t.text)))
        elif t.kind == "op" and t.text == "^^":                       # logical exclusive or (§5.9): on bools that is `!=`
            # `!=` binds tighter than `&&`, `^^` looser: refuse the one spelling where that would change the meaning silently
            for step in (-1, 1):
                depth, j = 0, k + step
                while 0 <= j < len(tokens):
                    text = tokens[j].text if tokens[j].kind == "op" else ""
                    if text in ("(", "[") if step == 1 else text in (")", "]"):
                        depth += 1
                    elif text in (")", "]") if step == 1 else text in ("(", "["):
                        if depth == 0:
                            break
                        depth -= 1
                    elif depth == 0 and text in (";", ",", "?", ":", "=", "||", "{", "}"):
                        break
                    elif depth == 0 and text == "&&":
                        raise TranslationError("`&&` next to `^^` without parentheses: write (a && b) ^^ c")
                    j += step
            out.append(Tok("op", "!="))
        elif t.kind == "op" and t.text == "." and _is_length_call(tokens, k) and _postfix_start(out) < len(out):
            # `name.length()`, `s.member.length()` of an array or vector (§4.1.9, §5.5) → length_of(name) (jit_runtime.hpp)
            start = _postfix_start(out)
            operand = _text(out[start:]).strip()
            del out[start:]
            out.append(Tok("ident", f"length_of({operand})"))
            k = _matching(tokens, _significant(tokens, _significant(tokens, k + 1) + 1), "(", ")")
        elif t.kind == "ident":
            nxt = _significant(tokens, k + 1)
            following = tokens[nxt].text if nxt < len(tokens) else ""
            before = _significant(tokens, k - 1, -1)
            taken = None
            if t.text in types and not uniform and nxt < len(tokens) and (following == "[" or tokens[nxt].kind == "ident"):
                taken = _array_declaration(tokens, k, types, structs, outs, out)
            if taken is not None:
                k = taken
            elif t.text in _DROPPED_QUALIFIERS:
                pass
            elif t.text == "uniform":
                uniform = True
                out.append(t)
            elif t.text == "layout" and following == "(":
                close = _matching(tokens, nxt, "(", ")")
                out.append(Tok("ws", "\n"*_text(tokens[k:close]).count("\n") or " "))
                k = close
            elif t.text in outs and following == "(" and not (before >= 0 and tokens[before].kind == "ident" and tokens[before].text in types):
                # a call of a function with `out` / `inout` parameters: a swizzle in such a position goes through sf_out (jit_runtime.hpp)
                close = _matching(tokens, nxt, "(", ")")
                out += [t, Tok("op", "(")]
                for position, argument in enumerate(_split_top_level(tokens[nxt + 1:close])):
                    inner = _rewrite_tokens(argument, structs, outs)
                    if position:
                        out.append(Tok("op", ","))
                    out += [Tok("ident", "sf_out"), Tok("op", "("), *inner, Tok("op", ")")] if position in outs[t.text] and _is_swizzle(argument) else inner
                out.append(Tok("op", ")"))
                k = close
            elif t.text in _CPP_ONLY_KEYWORDS:
                out.append(Tok("ident", t.text + "_"))
            elif t.text == "main":
                out.append(Tok("ident", "main_"))
            elif t.text in ("int", "uint") and following == "(":
                out.append(Tok("ident", "to_" + t.text))
            elif t.text in types and following == "[":
                # `T[n](a, b)` array constructor → `sf_arr_of<T>(a, b)` (jit_runtime.hpp; in a uniform's initialiser, which is only
                # read here, `{a, b}`);  `uniform T[n] name` → `T name[n]`
                close = _matching(tokens, nxt, "[", "]")
                after = _significant(tokens, close + 1)
                if after < len(tokens) and tokens[after].text == "(":
                    end = _matching(tokens, after, "(", ")")
                    inner = _rewrite_tokens(tokens[after + 1:end], structs, outs)
                    out += [Tok("op", "{")] if uniform else [Tok("ident", f"sf_arr_of<{t.text}>"), Tok("op", "(")]
                    out.extend(inner)
                    out.append(Tok("op", "}" if uniform else ")"))
                    k = end
                elif after < len(tokens) and tokens[after].kind == "ident":
                    out.append(t); out.append(Tok("ws", " ")); out.append(Tok("ident", tokens[after].text))
                    out.extend(_rewrite_tokens(tokens[nxt:close + 1], structs, outs))
                    k = after
                else:
                    out.append(t)
            else:
                out.append(t)
        else:
            out.append(t)
        k += 1
    return out


def _text(tokens: Iterable[Tok]) -> str:
    return "".join(t.text for t in tokens)


# ---- function heads ---------------------------------------------------------------------------------------------------

def _rewrite_parameters(tokens: list[Tok]) -> list[Tok]:
    """`in T a, out T b, inout T c, const in T d` → `T a, T& b, T& c, const T d`. Array parameters arrive as `sf_arr<T,3> e` and
    `out sf_arr<T,3> f` (_array_declaration) and follow the same rule: an `in` array is the function's own copy, as in GLSL"""
    out: list[Tok] = []
    parameter: list[Tok] = []

    def flush() -> None:
        words = [t for t in parameter if t.kind not in ("ws", "comment")]
        if not words:
            return
        reference = any(t.kind == "ident" and t.text in ("out", "inout") for t in words)
        constant = any(t.kind == "ident" and t.text == "const" for t in words)
        core = [t for t in words if not (t.kind == "ident" and t.text in ("in", "out", "inout", "const"))]
        type_, rest = core[0], core[1:]
        text = ("const " if constant and not reference else "") + type_.text + ("&" if reference else "") + " " + _text(rest)
        if out:
            out.append(Tok("op", ", "))
        out.append(Tok("ident", text))

    depth = 0
    for t in tokens:
        if t.kind == "op" and t.text in "([":
            depth += 1
        elif t.kind == "op" and t.text in ")]":
            depth -= 1
        if t.kind == "op" and t.text == "," and depth == 0:
            flush(); parameter = []
        else:
            parameter.append(t)
    flush()
    return out


# ---- the global scope -------------------------------------------------------------------------------------------------

_CONSTANT_TOKENS = re.compile(r"^[-+*/%()\s\d.eEfFuUxXa-fA-F<>&|^~!?:]*$")


class _Translator:
    def __init__(self, source: str, uniforms: list[tuple[str, str]]):
        self.source = source
        self.pipeline = list(uniforms)
        self.body: list[str] = []
        self.structs: set[str] = set()
        self.constants: set[str] = set()
        self.constant_values: dict[str, int] = {}                    # `const int N = 3;` → array sizes of uniform declarations
        self.declared_uniforms: list[tuple[str, str, str]] = []     # (type, name, default text)
        self.macros: list[str] = []
        self.identifiers: set[str] = set()

    # a statement of the global scope that ends in ';'
    def declaration(self, tokens: list[Tok]) -> str:
        first = _significant(tokens, 0)
        if first >= len(tokens):
            return _text(tokens)
        words = [t.text for t in tokens if t.kind == "ident"]
        head = tokens[first].text
        if head == "precision":
            return ""
        qualifiers = set()
        k = first
        while k < len(tokens) and (tokens[k].kind in ("ws",) or (tokens[k].kind == "ident" and tokens[k].text in ("uniform", "in", "out", "varying", "attribute", "const"))):
            if tokens[k].kind == "ident":
                qualifiers.add(tokens[k].text)
            k += 1
        rest = tokens[k:]
        if "uniform" in qualifiers:
            type_index = _significant(rest, 0)
            type_ = rest[type_index].text
            names = _text(rest[type_index + 1:-1])
            for part in self._split_commas(names):
                name, _, default = part.partition("=")
                self.declared_uniforms.append((type_, name.strip(), default.strip()))
            return ""
        if qualifiers & {"in", "out", "varying", "attribute"}:
            type_index = _significant(rest, 0)
            names = [n.strip() for n in self._split_commas(_text(rest[type_index + 1:-1]))]
            unknown = [n for n in names if n.split("[")[0].strip() not in BUILTIN_MEMBERS]
            return (f"\n{rest[type_index].text} {', '.join(unknown)};" if unknown else "")
        # prototype: `T name(params);` without an initialiser
        texts = [t.text for t in tokens if t.kind not in ("ws",)]
        if "=" not in texts and "(" in texts and texts[-2] == ")" and len(words) >= 2:
            return ""
        if head == "struct":
            return self.struct(tokens)
        text = _text(tokens)
        if "const" in qualifiers:
            type_index = _significant(rest, 0)
            type_ = rest[type_index].text
            if type_ in ("int", "float", "bool", "uint") and "[" not in texts:
                parts = self._split_commas(_text(rest[type_index + 1:-1]))
                constant = True
                for part in parts:
                    name, _, init = part.partition("=")
                    probe = re.sub(r"\b(?:%s|true|false)\b" % "|".join(sorted(self.constants) or ["__none__"]), "1", init)
                    probe = re.sub(r"\bto_u?int\b|\bfloat\b|\bbool\b", "", probe)
                    constant = constant and bool(init.strip()) and bool(_CONSTANT_TOKENS.match(probe))
                if constant:
                    for part in parts:
                        self.constants.add(part.partition("=")[0].strip())
                        if type_ == "int" and part.partition("=")[2].strip().isdigit():
                            self.constant_values[part.partition("=")[0].strip()] = int(part.partition("=")[2])
                    return f"\nstatic constexpr {type_} {', '.join(p.strip() for p in parts)};"
        return text

    @staticmethod
    def _split_commas(text: str) -> list[str]:
        parts, depth, current = [], 0, ""
        for ch in text:
            if ch in "([{":
                depth += 1
            elif ch in ")]}":
                depth -= 1
            if ch == "," and depth == 0:
                parts.append(current); current = ""
            else:
                current += ch
        if current.strip():
            parts.append(current)
        return parts

    def struct(self, tokens: list[Tok]) -> str:
        """`==` and `!=` of two structs compare member by member (§5.9): C++20 writes that comparison itself"""
        words = [k for k, t in enumerate(tokens) if t.kind not in ("ws", "comment")]
        open_ = next((k for k in words if tokens[k].kind == "op" and tokens[k].text == "{"), None)
        if open_ is None or len(words) < 3 or tokens[words[1]].kind != "ident" or words[2] != open_:
            return _text(tokens)
        close = _matching(tokens, open_, "{", "}")
        return _text(tokens[:close]) + f" SF_HD bool operator==(const {tokens[words[1]].text}&) const = default; " + _text(tokens[close:])

    def function(self, head: list[Tok], body: list[Tok], line: int) -> str:
        """`line`: the fragment's line of the body's opening brace. A `#line` there (and after every directive inside the body, which
        takes lines of its own here) keeps `__LINE__` (§3.3) and the compiler's messages on the lines of the GLSL text"""
        open_ = next(i for i, t in enumerate(head) if t.kind == "op" and t.text == "(")
        close = _matching(head, open_, "(", ")")
        before = head[:open_]
        return_type = next((t.text for t in before if t.kind == "ident"), "void")
        parameters = _rewrite_parameters(head[open_ + 1:close])
        if _text(parameters).strip() == "void":
            parameters = []
        body_text = self.function_body(body, return_type, line)
        return "\nSF_HD " + _text(before).lstrip() + "(" + _text(parameters) + ")" + _text(head[close + 1:]).rstrip() + f"\n#line {line}\n" + body_text

    def function_body(self, body: list[Tok], return_type: str, line: int) -> str:
        out = []
        for t in body:
            line += t.text.count("\n")
            if t.kind == "ident" and t.text == "discard":
                # the invocation ends in GLSL; here the flag makes the result transparent whatever the callers still compute
                out.append("{ discarded_ = true; return; }" if return_type == "void" else "{ discarded_ = true; return {}; }")
            elif t.kind == "pp":
                out.append("\n" + self.preprocessor(t.text).strip("\n") + f"\n#line {line + 1}")
            else:
                out.append(t.text)
        return "".join(out)

    def preprocessor(self, text: str) -> str:
        text = re.sub(r"\\\r?\n", " ", text)                       # a continued line (§3.1) is one line
        stripped = text.strip()
        directive = re.match(r"#\s*(\w+)", stripped)
        name = directive.group(1) if directive else ""
        if name in ("version", "extension", "pragma", "line", "include"):
            return ""
        if name == "define":
            match = re.match(r"(\s*#\s*define\s+)(\w+)(.*)$", text, re.S)
            if match:
                self.macros.append(match.group(2))
                rewritten = _text(_rewrite_tokens(tokenize(match.group(3)), self.structs))
                return match.group(1) + (match.group(2) + "_" if match.group(2) in _CPP_ONLY_KEYWORDS else match.group(2)) + rewritten
        return text

    def run(self) -> Translation:
        raw = tokenize(self.source)
        # names the fragment can reach: those of its code, and those of the macros it reaches (a texture's `#define name
        # name0x0` must not make the sampler active unless `name` is used)
        self.identifiers = {t.text for t in raw if t.kind == "ident"}
        macros: dict[str, set[str]] = {}
        for t in raw:
            if t.kind == "pp":
                define = re.match(r"\s*#\s*define\s+(\w+)(?:\([^)]*\))?(.*)$", t.text, re.S)
                if define:
                    macros.setdefault(define.group(1), set()).update(re.findall(r"[A-Za-z_]\w*", define.group(2)))
                else:
                    self.identifiers |= set(re.findall(r"[A-Za-z_]\w*", t.text))
        grown = True
        while grown:
            grown = False
            for name, names in macros.items():
                if name in self.identifiers and not names <= self.identifiers:
                    self.identifiers |= names
                    grown = True
        # struct names first: they are types for the array rewrites
        for k, t in enumerate(raw):
            if t.kind == "ident" and t.text == "struct":
                nxt = _significant(raw, k + 1)
                if nxt < len(raw) and raw[nxt].kind == "ident":
                    self.structs.add(raw[nxt].text)
        names = {t.text for t in raw if t.kind == "ident"}
        missing = sorted(name for name in names if re.fullmatch(r"mat[234]x[234]|[iu]?sampler(?:[123]D|Cube|Buffer|2DRect|2DMS)(?:Array)?(?:Shadow)?", name)
                         and name not in _TYPES)
        if missing:
            raise TranslationError(f"type {', '.join(missing)}: only float, int, uint and bool scalars and vectors, square float matrices and sampler2D exist here")
        for word in sorted(_CPP_ONLY_KEYWORDS & names):
            if word + "_" in names:
                raise TranslationError(f"identifiers '{word}' and '{word}_': '{word}' is a C++ keyword and is renamed to '{word}_' here; rename one of the two")
        tokens = _rewrite_tokens(raw, self.structs, out_parameters(raw, _TYPES | self.structs))
        k, statement = 0, []
        lines = [1]                                                # lines[k]: the fragment's line tokens[k] starts on (the rewrites keep newlines)
        for t in tokens:
            lines.append(lines[-1] + t.text.count("\n"))
        while k < len(tokens):
            t = tokens[k]
            if t.kind == "pp":
                self.body.append(_text(statement)); statement = []
                self.body.append("\n" + self.preprocessor(t.text).strip("\n") + "\n")
            elif t.kind == "op" and t.text == ";":
                statement.append(t)
                self.body.append(self.declaration(statement)); statement = []
            elif t.kind == "op" and t.text == "{":
                end = _matching(tokens, k, "{", "}")
                texts = [s.text for s in statement if s.kind != "ws"]
                if "=" in texts:                                   # brace initialiser of a global: part of the statement
                    statement.extend(tokens[k:end + 1])
                elif texts and texts[0] == "struct":               # struct definition (up to its ';')
                    statement.extend(tokens[k:end + 1])
                elif "(" in texts:                                 # function definition
                    self.body.append(self.function(statement, tokens[k:end + 1], lines[k])); statement = []
                else:
                    raise TranslationError(f"unexpected block after {_text(statement).strip()!r}")
                k = end
            else:
                statement.append(t)
            k += 1
        if _text(statement).strip():
            raise TranslationError(f"unterminated declaration: {_text(statement).strip()[:60]!r}")
        return self.assemble()

    def _array_length(self, text: str) -> int:
        if text.isdigit():
            return int(text)
        value = self.constant_values.get(text)
        if value is None:
            raise TranslationError(f"array size '{text}' is not an integer literal or a literal `const int`")
        return int(value)

    def assemble(self) -> Translation:
        bindings: list[Binding] = []
        members: list[str] = []
        loads: list[str] = []
        seen: set[str] = set()
        next_float = 0
        free_samplers = [s for s in range(TEX_SLOTS) if s not in FIXED_SAMPLER_SLOTS.values()]
        wanted = [(type_, name, "") for (type_, name) in self.pipeline] + self.declared_uniforms
        declared_names = {name for (_, name, _) in self.declared_uniforms}
        for (type_, name, default) in wanted:
            if name in seen or name in BUILTIN_MEMBERS:
                continue
            if name not in self.identifiers and name not in declared_names:
                continue                                           # inactive uniform: the driver would have removed it as well
            seen.add(name)
            if type_ == "sampler2D":
                # the engine names a texture's newest box `<name>0x0` (texture.py:346-347) and #defines the plain name to it
                plain = name[:-3] if name.endswith("0x0") else name
                if plain in FIXED_SAMPLER_SLOTS:
                    slot = FIXED_SAMPLER_SLOTS[plain]
                elif free_samplers:
                    slot = free_samplers.pop(0)
                else:
                    raise TranslationError(f"more than {TEX_SLOTS} samplers")
                bindings.append(Binding(name, type_, slot))
                members.append(f"    sampler2D {name};")
                loads.append(f"{name} = sampler_({slot});")
                continue
            length = None                                          # `uniform T name[N]`: N elements, bound as name[0] … name[N-1]
            array = re.fullmatch(r"(\w+)\s*\[\s*(\w+)\s*\]", name)
            if array:
                name = array.group(1)
                length = self._array_length(array.group(2))
            elif "[" in name:
                raise TranslationError(f"uniform {name}: only one-dimensional arrays with a literal or constant size are supported")
            if type_ not in _UNIFORM_COUNTS:
                raise TranslationError(f"uniform {name}: type {type_} is not supported")
            count, integer = _UNIFORM_COUNTS[type_]
            if next_float + count*(length or 1) > USER_SLOTS:
                raise TranslationError(f"more than {USER_SLOTS} floats of uniforms")
            defaults = _constant_initialiser(type_, count, length, default, name) if default else None

            def load(target: str, first: int) -> str:
                getter = "user_int_" if integer else "user_"
                values = ", ".join(f"{getter}({first + i})" for i in range(count))
                if type_ == "bool":
                    return f"{target} = user_int_({first}) != 0;"
                if type_ == "uint":
                    return f"{target} = (uint)user_int_({first});"
                if count == 1:
                    return f"{target} = {values};"
                return f"{target} = {type_}({values});"

            if length is None:
                members.append(f"    {type_} {name};")
                loads.append(load(name, next_float))
                bindings.append(Binding(name, type_, next_float, count, integer, default=defaults[0] if defaults else None))
                next_float += count
            else:
                members.append(f"    sf_arr<{type_},{length}> {name};")
                for index in range(length):
                    loads.append(load(f"{name}[{index}]", next_float))
                    bindings.append(Binding(f"{name}[{index}]", type_, next_float, count, integer,
                                            default=defaults[index] if defaults else None, array=name))
                    next_float += count
        code = "".join(self.body)
        undefs = "".join(f"#undef {m}\n" for m in dict.fromkeys(self.macros))
        derivatives = bool(self.identifiers & {'dFdx', 'dFdy', 'fwidth'})
        audio = bool(self.identifiers & AUDIO_UNIFORMS)
        tiled = None if derivatives else _sampler_worth_a_tile(code, [b for b in bindings if b.type == "sampler2D"])
        cpp = ("// generated by shaderflow_amd/glsl2hip.py from a GLSL fragment\n"
               + (f"#define SF_JIT_TILE_SLOT {tiled.slot}      // {tiled.name}\n" if tiled else "") +
               "#include \"jit_runtime.hpp\"\n"
               "namespace sf { namespace rt {\n"
               "struct Fragment : FragmentBase {\n" + "\n".join(members) + "\n"
               "    SF_HD void load_user_() { " + " ".join(loads) + " }\n"
               "// ---- translated fragment ----\n" + code + "\n"
               "// ---- end of translated fragment ----\n"
               "};\n"
               "}}\n" + undefs +
               f"#define SF_JIT_DERIVATIVES {int(derivatives)}\n"
               f"#define SF_JIT_AUDIO {int(audio)}\n"
               "SF_JIT_ENTRY_POINTS(sf::rt::Fragment)\n")
        return Translation(cpp, bindings, tiled.name if tiled else None)


# the lookups the tile can serve: level 0 with the plain filter, moved by an offset or not (jit_runtime.hpp tiled_texture)
_TEXTURE_CALLS = r"(?:texture|textureLod|textureOffset|textureLodOffset|textureProj|textureProjOffset|gtexture|gmtexture|stexture|astexture|agtexture|agmtexture)"


def _closing_in_text(code: str, at: int, opening: str, closing: str) -> int:
    """index just past the bracket that closes the one at `at`"""
    depth = 0
    for k in range(at, len(code)):
        if code[k] == opening:
            depth += 1
        elif code[k] == closing:
            depth -= 1
            if depth == 0:
                return k + 1
    return len(code)


def _loop_bodies(code: str) -> list[tuple[int, int]]:
    """(first, last) text ranges of the header and body of every for / while loop"""
    ranges = []
    for match in re.finditer(r"\b(?:for|while)\s*\(", code):
        header_end = _closing_in_text(code, match.end() - 1, "(", ")")
        rest = code[header_end:]
        body = header_end + len(rest) - len(rest.lstrip())
        if body < len(code) and code[body] == "{":
            end = _closing_in_text(code, body, "{", "}")
        else:
            semicolon = code.find(";", body)
            end = len(code) if semicolon < 0 else semicolon + 1
        ranges.append((match.start(), end))
    return ranges


def _sampler_worth_a_tile(code: str, samplers: list[Binding]) -> Optional[Binding]:
    """The sampler a tap-heavy fragment reads most (a blur or feedback kernel: taps inside the text of a loop, or eight and more
    written out), or None. SHADERFLOW_JIT_TILE=0 turns the tile off, =<sampler name> forces it for that sampler.

    The tile costs one extra evaluation of the fragment per block (jit_runtime.hpp JitShader::setup) and never changes a
    result, so the choice is about speed only: a single tap does not pay for the probe. Taps are `texture` and the prelude's
    helpers, `textureOffset` (a blur written with offsets: the recorded box widens by them), `textureProj[Offset]`, and
    `textureLod[Offset]` — on a texture without a chain a lod selects nothing and the tap is served from the tile; on a mipmapped
    one every lookup bypasses it (the tile holds level 0 only)."""
    wish = os.environ.get("SHADERFLOW_JIT_TILE", "1")
    if wish.lower() in ("0", "off", "false", "no"):
        return None
    forced = [b for b in samplers if b.name == wish or (b.name.endswith("0x0") and b.name[:-3] == wish)]
    if forced:
        return forced[0]
    loops = _loop_bodies(code)
    in_loop = lambda at: any(first <= at < last for (first, last) in loops)
    weight = lambda at: 16 if in_loop(at) else 1
    tap_on = lambda names: re.compile(rf"\b{_TEXTURE_CALLS}\s*\(\s*(?:{'|'.join(map(re.escape, names))})\b")
    # helper functions that tap a sampler PARAMETER (`vec4 blur(sampler2D tex, vec2 uv) { for (…) … texture(tex, …) }`): the taps
    # count for whatever sampler a call passes in that position, once more heavily when the call itself sits in a loop
    helpers = []                                               # (name, position of the sampler parameter, weight of its taps)
    for definition in re.finditer(r"\bSF_HD\s+[\w:<>,]+\s+(\w+)\s*\(([^()]*)\)\s*(?:const\s*)?(?:#line \d+\s*)?\{", code):
        body_end = _closing_in_text(code, definition.end() - 1, "{", "}")
        for position, parameter in enumerate(_split_arguments(definition.group(2))):
            declared = re.fullmatch(r"\s*(?:const\s+)?sampler2D\s*&?\s*(\w+)\s*", parameter)
            if declared:
                taps = sum(weight(m.start()) for m in tap_on([declared.group(1)]).finditer(code, definition.end(), body_end))
                if taps:
                    helpers.append((definition.group(1), position, taps))
    best, best_score = None, 0
    for binding in samplers:
        names = {binding.name, binding.name[:-3] if binding.name.endswith("0x0") else binding.name}
        score = sum(weight(m.start()) for m in tap_on(names).finditer(code))
        for (helper, position, taps) in helpers:
            for call in re.finditer(rf"\b{re.escape(helper)}\s*\(", code):
                arguments = _split_arguments(code[call.end():_closing_in_text(code, call.end() - 1, "(", ")") - 1])
                if position < len(arguments) and arguments[position].strip() in names:
                    score += taps*weight(call.start())
        if score > best_score:
            best, best_score = binding, score
    return best if best_score >= 8 else None


_SCALAR_OF = {"float": float, "int": int, "uint": int, "bool": bool}


def _constant_scalar(text: str, name: str) -> float:
    """A literal arithmetic expression of a uniform initialiser → its value (`-0.5`, `2.0*3.0`, `1e-3`, `true`, `3u`)"""
    import ast
    cleaned = re.sub(r"(?<=[0-9.])(?:lf|LF|[fFuU])\b", "", text.strip())
    cleaned = re.sub(r"\btrue\b", "1", re.sub(r"\bfalse\b", "0", cleaned))
    cleaned = re.sub(r"\b(?:float|int|uint|bool)\s*\(", "(", cleaned)
    try:
        tree = ast.parse(cleaned, mode="eval")
    except SyntaxError:
        raise TranslationError(f"uniform {name}: initialiser '{text}' is not a literal constant expression") from None
    allowed = (ast.Expression, ast.BinOp, ast.UnaryOp, ast.Constant, ast.Add, ast.Sub, ast.Mult, ast.Div, ast.USub, ast.UAdd)
    if not all(isinstance(node, allowed) for node in ast.walk(tree)):
        raise TranslationError(f"uniform {name}: initialiser '{text}' is not a literal constant expression")
    import builtins                                            # this module defines its own compile()
    return float(eval(builtins.compile(tree, "<initialiser>", "eval"), {"__builtins__": {}}))


def _split_arguments(text: str) -> list[str]:
    parts, depth, current = [], 0, ""
    for ch in text:
        if ch in "([":
            depth += 1
        elif ch in ")]":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(current)
            current = ""
        else:
            current += ch
    if current.strip():
        parts.append(current)
    return parts


def _constant_value(type_: str, count: int, text: str, name: str) -> tuple:
    """`T(…)` or a scalar expression → `count` numbers (vector constructors splat a single argument, matrices put it on the diagonal)"""
    text = text.strip()
    constructor = re.fullmatch(rf"{type_}\s*\((.*)\)", text, re.S)
    if count == 1:
        return (_constant_scalar(constructor.group(1) if constructor else text, name),)
    if not constructor:
        raise TranslationError(f"uniform {name}: initialiser '{text}' must be a {type_}(…) constructor of literals")
    arguments = [_constant_scalar(a, name) for a in _split_arguments(constructor.group(1))]
    if len(arguments) == 1:
        if type_.startswith("mat"):
            side = int(type_[3])
            return tuple(arguments[0] if (k % (side + 1) == 0) else 0.0 for k in range(count))
        return tuple(arguments*count)
    if len(arguments) != count:
        raise TranslationError(f"uniform {name}: {type_} initialiser with {len(arguments)} components")
    return tuple(arguments)


def _constant_initialiser(type_: str, count: int, length: Optional[int], text: str, name: str) -> list[tuple]:
    """The initialiser of a uniform declaration as one tuple per element (one element for a non-array)"""
    if length is None:
        return [_constant_value(type_, count, text, name)]
    # (array constructors reach this point already rewritten to C++ brace lists)
    array = re.fullmatch(rf"{type_}\s*\[\s*\w*\s*\]\s*\((.*)\)", text.strip(), re.S) or re.fullmatch(r"\{(.*)\}", text.strip(), re.S)
    if not array:
        raise TranslationError(f"uniform {name}: an array initialiser must be written {type_}[](…)")
    elements = _split_arguments(array.group(1))
    if len(elements) != length:
        raise TranslationError(f"uniform {name}: {len(elements)} initialisers for {length} elements")
    return [_constant_value(type_, count, element, name) for element in elements]


def translate(source: str, uniforms: Iterable[tuple[str, str]] = ()) -> Translation:
    """GLSL fragment text (defines + includes + content, without the `uniform` declarations the engine generates) and the
    pipeline's `(type, name)` pairs → C++ translation unit + the bindings of its uniforms and samplers"""
    return _Translator(source, list(uniforms)).run()


# ---- compile ----------------------------------------------------------------------------------------------------------

_fingerprint: Optional[str] = None


def runtime_fingerprint() -> str:
    """Hash of the headers a code object is compiled against (its RenderArgs layout must match the library's)"""
    global _fingerprint
    if _fingerprint is None:
        digest = hashlib.sha256()
        for name in ("sfmath.hpp", "glsl.hpp", "fragments.hpp", "render_kernels.hpp", "jit_runtime.hpp", "jit_swizzles.inc", "jit_intvec.inc",
                     "uniform_table.hpp"):
            digest.update((CSRC/name).read_bytes())
        digest.update(" ".join(FLAGS).encode())
        # …and the layout the LOADED library was built with (a variant library built with other switches, or headers edited since it
        # was built, must not pick up code objects cached for another layout; sfx_program_load checks the same value)
        try:
            from shaderflow_amd import _native
            digest.update(str(_native.lib().sfx_abi_layout()).encode())
        except Exception:                                      # no library yet (host-only translation tests): headers alone
            pass
        _fingerprint = digest.hexdigest()
    return _fingerprint


def cache_directory() -> Path:
    root = os.environ.get("SHADERFLOW_JIT_CACHE")
    if root:
        return Path(root)
    return Path(os.environ.get("XDG_CACHE_HOME", Path.home()/".cache"))/"shaderflow_amd"/"jit"


def compile(translation: Translation, *, cache: Optional[Path] = None, timeout: float = 300.0) -> bytes:
    """Translation → gfx950 code object (bytes), through the on-disk cache"""
    cache = Path(cache) if cache else cache_directory()
    cache.mkdir(parents=True, exist_ok=True)
    target = cache/f"{translation.key}.hsaco"
    if target.exists():
        return target.read_bytes()
    unit = cache/f"{translation.key}.hip"
    unit.write_text(translation.cpp)
    temporary = cache/f"{translation.key}.{os.getpid()}.tmp"
    command = [HIPCC, *FLAGS, f"-I{CSRC}", "--genco", str(unit), "-o", str(temporary)]
    try:
        done = subprocess.run(command, capture_output=True, text=True, timeout=timeout)
    except FileNotFoundError as error:
        raise CompileError(f"hipcc not found ({HIPCC}): fragments outside the registry need the ROCm compiler at run time") from error
    except subprocess.TimeoutExpired as error:
        raise CompileError(f"hipcc timed out after {timeout:.0f} s") from error
    if done.returncode != 0 or not temporary.exists():
        temporary.unlink(missing_ok=True)
        raise CompileError(f"hipcc failed ({unit}):\n{done.stderr[-4000:]}")
    os.replace(temporary, target)
    return target.read_bytes()
