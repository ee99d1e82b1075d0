"""
glsl2hip — fragments that are not in the kernel registry: GLSL 3.30 → HIP C++ → gfx950 code object.

The reference gives the assembled GLSL to the OpenGL driver (shader.py:190-239 builds the text, :313-349 compiles it
with `opengl.program`, falling back to `missing.glsl` on errors). Without a driver the same job is done in two steps:

1. `translate()` rewrites the fragment token by token into the body of a C++ struct that derives from
   `sf::rt::FragmentBase` (csrc/jit_runtime.hpp): globals and uniforms become members, functions become member
   functions, `main` becomes `main_`. It cuts the fragment's own tokens into the items of the global scope first (directives,
   declarations, prototypes, functions), rewrites and emits each by its kind, and assembles the struct around them. GLSL and C++ share almost all of their expression and statement syntax; the
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

import ast
import bisect
import builtins
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

    def is_op(self, *texts: str) -> bool:
        """the operator `x`, or one of these operators"""
        return self.kind == "op" and self.text in texts


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
    return text + "f" if "." in text or "e" in text.lower() else text


def _matching(tokens: list[Tok], start: int, open_: str, close: str) -> int:
    """index of the token closing the bracket opened at `start`"""
    depth = 0
    for k in range(start, len(tokens)):
        if tokens[k].is_op(open_, close):
            depth += 1 if tokens[k].text == open_ else -1
            if depth == 0:
                return k
    raise TranslationError(f"unbalanced {open_!r}")


_BRACKETS = (("(", "[", "{"), (")", "]", "}"))


def _scan(tokens: list[Tok], start: int, step: int, stops: tuple = ()) -> int:
    """index of the first token from `start` (inclusive) in direction `step` that is one of the operators `stops` outside every
    bracket passed on the way, or the bracket that closes the enclosing one; len(tokens) / -1 if there is none"""
    opening, closing = _BRACKETS[::step]
    depth, k = 0, start
    while 0 <= k < len(tokens):
        text = tokens[k].text if tokens[k].kind == "op" else None
        if text in opening:
            depth += 1
        elif text in closing:
            if depth == 0:
                break
            depth -= 1
        elif depth == 0 and text in stops:
            break
        k += step
    return k


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
    parts, start, k = [], 0, _scan(tokens, 0, 1, (",",))
    while k < len(tokens) and tokens[k].is_op(","):
        parts.append(tokens[start:k])
        start = k + 1
        k = _scan(tokens, start, 1, (",",))
    if any(t.kind not in ("ws", "comment") for t in tokens[start:]):
        parts.append(tokens[start:])
    return parts


def _postfix_start(out: list[Tok]) -> int:
    """index in `out` where the postfix expression that ends `out` begins: `s.w`, `a[1].b`, `f(x)[2]`, `name`"""
    k = len(out)
    while True:
        j = _significant(out, k - 1, -1)
        if j >= 0 and out[j].is_op(")", "]"):
            k = _scan(out, j - 1, -1)
            if k < 0:
                raise TranslationError("unbalanced bracket before .length()")
        elif j >= 0 and out[j].kind == "ident" and out[j].text not in _STATEMENT_WORDS:
            k = _significant(out, j - 1, -1)
            if k < 0 or not out[k].is_op("."):
                return j
        else:
            return k


def _is_swizzle(tokens: list[Tok]) -> bool:
    """the expression ends in a swizzle of two to four components (`v.zw`, `m[1].yx`)"""
    last = _significant(tokens, len(tokens) - 1, -1)
    dot = _significant(tokens, last - 1, -1) if last > 0 else -1
    return dot >= 0 and tokens[last].kind == "ident" and bool(_SWIZZLE.fullmatch(tokens[last].text)) and tokens[dot].is_op(".")


def _declarators(tokens: list[Tok], start: int, types: set[str]) -> tuple[list, int]:
    """the declarators from the name at tokens[start]: [(name, tokens of `[size]` or None, tokens of the initialiser or None)] and
    the index of the token that ends them (`;`, `)`, the comma before the next parameter, `(` of a function head)"""
    found = []
    k = start
    while True:
        j = _significant(tokens, k + 1)
        size = initialiser = None
        if j < len(tokens) and tokens[j].is_op("["):
            close = _matching(tokens, j, "[", "]")
            size = tokens[j + 1:close]
            j = _significant(tokens, close + 1)
        if j < len(tokens) and tokens[j].is_op("="):
            end = _scan(tokens, j + 1, 1, (",", ";"))
            initialiser = tokens[j + 1:end]
            j = end
        found.append((tokens[k], size, initialiser))
        if j < len(tokens) and tokens[j].is_op(","):
            name = _significant(tokens, j + 1)
            after = _significant(tokens, name + 1)
            if (after < len(tokens) and tokens[name].kind == "ident" and tokens[name].text not in types | _QUALIFIERS
                    and tokens[after].is_op("[", "=", ",", ";")):
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
            length = "".join(_text(_rewrite_tokens(bound, structs, outs)).split()) or _constructor_length(name.text, initialiser)
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


def _rewrite_tokens(tokens: list[Tok], structs: set[str], outs: Optional[dict] = None) -> list[Tok]:
    out: list[Tok] = []
    k = 0
    types = _TYPES | structs
    outs = outs or {}
    while k < len(tokens):
        t = tokens[k]
        if t.kind == "comment":
            out.append(Tok("ws", "\n"*t.text.count("\n") or " "))
        elif t.kind == "number":
            out.append(Tok("number", _float_literal(t.text)))
        elif t.is_op("^^"):                                           # logical exclusive or (§5.9): on bools that is `!=`
            # `!=` binds tighter than `&&`, `^^` looser: refuse the one spelling where that would change the meaning silently
            for step in (-1, 1):
                j = _scan(tokens, k + step, step, (";", ",", "?", ":", "=", "||", "&&"))
                if 0 <= j < len(tokens) and tokens[j].is_op("&&"):
                    raise TranslationError("`&&` next to `^^` without parentheses: write (a && b) ^^ c")
            out.append(Tok("op", "!="))
        elif t.is_op(".") and _is_length_call(tokens, k) and _postfix_start(out) < len(out):
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
            if t.text in types and nxt < len(tokens) and (following == "[" or tokens[nxt].kind == "ident"):
                taken = _array_declaration(tokens, k, types, structs, outs, out)
            if taken is not None:
                k = taken
            elif t.text in _DROPPED_QUALIFIERS:
                pass
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
            elif t.text in _CPP_ONLY_KEYWORDS or t.text == "main":
                out.append(Tok("ident", t.text + "_"))
            elif t.text in ("int", "uint") and following == "(":
                out.append(Tok("ident", "to_" + t.text))
            elif t.text in types and following == "[":
                # `T[n](a, b)` array constructor → `sf_arr_of<T>(a, b)` (jit_runtime.hpp)
                close = _matching(tokens, nxt, "[", "]")
                after = _significant(tokens, close + 1)
                if after < len(tokens) and tokens[after].text == "(":
                    end = _matching(tokens, after, "(", ")")
                    out += [Tok("ident", f"sf_arr_of<{t.text}>"), Tok("op", "("), *_rewrite_tokens(tokens[after + 1:end], structs, outs), Tok("op", ")")]
                    k = end
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

def _rewrite_parameters(parameters: list[list[Tok]]) -> str:
    """`in T a, out T b, inout T c, const in T d` → `T a, T& b, T& c, const T d`. Array parameters arrive as `sf_arr<T,3> e` and
    `out sf_arr<T,3> f` (_array_declaration) and follow the same rule: an `in` array is the function's own copy, as in GLSL"""
    out = []
    for parameter in parameters:
        words = [t for t in parameter if t.kind not in ("ws", "comment")]
        if not words:
            continue
        reference = any(t.kind == "ident" and t.text in ("out", "inout") for t in words)
        constant = any(t.kind == "ident" and t.text == "const" for t in words)
        core = [t for t in words if not (t.kind == "ident" and t.text in ("in", "out", "inout", "const"))]
        out.append(("const " if constant and not reference else "") + core[0].text + ("&" if reference else "") + " " + _text(core[1:]))
    return ", ".join(out)


# ---- the global scope -------------------------------------------------------------------------------------------------

_STORAGE_QUALIFIERS = {"uniform", "in", "out", "varying", "attribute", "const"}
_LITERAL_OPERATORS = set("-+*/%()<>&|^~!?:.")
_LITERAL_WORD = set("0123456789abcdefABCDEFuUxX")                  # the characters of a number: a word spelled with them alone counts as one


@dataclass
class _Item:
    """One piece of the global scope, cut from the fragment's own tokens"""
    kind: str                                    # "directive", "declaration" (… `;`), "prototype", "function", "text" (what a directive cuts short)
    tokens: list[Tok]                            # all of it; of a function or prototype what stands before the `(`
    qualifiers: set = field(default_factory=set)         # of a declaration: its storage qualifiers, the index of its type in `tokens`
    type: int = 0
    parameters: list = field(default_factory=list)       # of a function or prototype: one token run each
    tail: list = field(default_factory=list)     # of a function: what stands between `)` and `{`, `{` … `}`, the fragment's line of that `{`
    body: list = field(default_factory=list)
    line: int = 0


def _storage(tokens: list[Tok]) -> tuple[set, int]:
    """the storage qualifiers a declaration begins with and the index of what follows them, its type; the qualifiers C++ lacks and
    `layout(…)` are passed over"""
    qualifiers, k = set(), 0
    while k < len(tokens):
        t, nxt = tokens[k], _significant(tokens, k + 1)
        if t.kind == "ident" and t.text in _STORAGE_QUALIFIERS:
            qualifiers.add(t.text)
        elif t.kind == "ident" and t.text == "layout" and nxt < len(tokens) and tokens[nxt].is_op("("):
            k = _matching(tokens, nxt, "(", ")")
        elif not (t.kind in ("ws", "comment") or (t.kind == "ident" and t.text in _DROPPED_QUALIFIERS)):
            break
        k += 1
    return qualifiers, k


def out_parameters(items: list[_Item], types: set[str]) -> dict[str, set[int]]:
    """function name → positions of its `out` / `inout` parameters (every overload of a name together, prototypes too), the built-ins'
    included. A function counts where a type stands before its name (`T name(`, `T[n] name(`), not one a macro names (`REAL name(`)"""
    found = {name: set(positions) for name, positions in _BUILTIN_OUT_PARAMETERS.items()}
    for item in items:
        positions = {i for i, p in enumerate(item.parameters) if any(w.kind == "ident" and w.text in ("out", "inout") for w in p)}
        name = _significant(item.tokens, len(item.tokens) - 1, -1)
        word = _significant(item.tokens, name - 1, -1)
        if word >= 0 and item.tokens[word].is_op("]"):
            word = _significant(item.tokens, _scan(item.tokens, word - 1, -1) - 1, -1)
        if positions and word >= 0 and item.tokens[word].text in types and item.tokens[name].kind == "ident":
            found.setdefault(item.tokens[name].text, set()).update(positions)
    return found


class _Translator:
    def __init__(self, source: str, uniforms: list[tuple[str, str]]):
        self.source = source
        self.pipeline = list(uniforms)
        self.body: list[str] = []
        self.structs: set[str] = set()
        self.constants: set[str] = set()
        self.constant_values: dict[str, int] = {}                    # `const int N = 3;` → array sizes of uniform declarations
        self.declared_uniforms: list[tuple] = []                    # (type, tokens of the declarator, those of the initialiser or None)
        self.macros: list[str] = []
        self.identifiers: set[str] = set()
        self.outs: dict[str, set[int]] = {}
        # for the tile heuristic: the functions that take a sampler2D (name, [(position, parameter)], first and last offset of the body in
        # the emitted text)
        self.helpers: list[tuple] = []

    def rewritten(self, tokens: list[Tok]) -> list[Tok]:
        return _rewrite_tokens(tokens, self.structs, self.outs)

    def text(self, tokens: list[Tok]) -> str:
        return _text(self.rewritten(tokens))

    # ---- cut: the raw tokens → items

    def statement(self, tokens: list[Tok]) -> _Item:
        """what ends in `;` at the global scope"""
        qualifiers, k = _storage(tokens)
        words = [t for t in tokens[k:] if t.kind not in ("ws", "comment")]
        open_ = next((j for j in range(k, len(tokens)) if tokens[j].is_op("(")), None)
        declares = qualifiers & (_STORAGE_QUALIFIERS - {"const"}) or any(t.is_op("=") for t in words)
        named = len(qualifiers) + sum(t.kind == "ident" for t in words) >= 2
        if open_ is not None and not declares and named and words[-2].is_op(")"):        # prototype: `T name(params);`
            return _Item("prototype", tokens[:open_], qualifiers, k, _split_top_level(tokens[open_ + 1:_matching(tokens, open_, "(", ")")]))
        return _Item("declaration", tokens, qualifiers, k)

    def cut(self, raw: list[Tok]) -> list[_Item]:
        items: list[_Item] = []
        lines = [1]                                                # lines[k]: the fragment's line raw[k] starts on
        for t in raw:
            lines.append(lines[-1] + t.text.count("\n"))
        k = start = 0
        while k < len(raw):
            t = raw[k]
            if t.kind == "pp":
                items += [_Item("text", raw[start:k]), _Item("directive", [t])]
                start = k + 1
            elif t.is_op(";"):
                items.append(self.statement(raw[start:k + 1]))
                start = k + 1
            elif t.is_op("{"):
                end = _matching(raw, k, "{", "}")
                head = raw[start:k]
                words = [s for s in head if s.kind not in ("ws", "comment")]
                # a brace initialiser of a global and a struct definition (up to its ';') are part of the statement
                if not any(s.is_op("=") for s in words) and not (words and words[0].text == "struct"):
                    first = _storage(head)[1]
                    open_ = next((j for j in range(first, len(head)) if head[j].is_op("(")), None)
                    if open_ is None:
                        raise TranslationError(f"unexpected block after {_text(_rewrite_tokens(head, self.structs)).strip()!r}")
                    close = _matching(head, open_, "(", ")")
                    items.append(_Item("function", head[:open_], parameters=_split_top_level(head[open_ + 1:close]), tail=head[close + 1:],
                                       body=raw[k:end + 1], line=lines[k]))
                    start = end + 1
                k = end
            k += 1
        if _significant(raw, start) < len(raw):
            raise TranslationError(f"unterminated declaration: {_text(raw[start:]).strip()[:60]!r}")
        return items

    # ---- rewrite and emit, by kind

    def declaration(self, item: _Item) -> str:
        tokens = item.tokens
        head, type_ = tokens[_significant(tokens, 0)].text, tokens[item.type].text
        if head == "precision" or item.kind == "prototype":
            return ""
        first, prefix = _significant(tokens, item.type + 1), []
        if "uniform" in item.qualifiers and type_ in _TYPES | self.structs and first < len(tokens) and tokens[first].is_op("["):
            close = _matching(tokens, first, "[", "]")         # `uniform T[n] a, b` is `uniform T a[n], b`: b is no array here
            first, prefix = close + 1, tokens[first:close + 1]
        # the declarators, and in each where its `=` stands
        parts = [(part, next((k for k, t in enumerate(part) if t.is_op("=")), len(part))) for part in _split_top_level(tokens[first:-1])]
        if "uniform" in item.qualifiers:
            for (part, eq) in parts:
                name = min(_significant(part, 0) + 1, eq)
                # (the name behind `T[n]` keeps its spelling, that of a C++ keyword too)
                spelled = [part[name - 1]] if prefix and name else self.rewritten(part[:name])
                spelled, prefix = spelled + self.rewritten(prefix + part[name:eq]), []
                self.declared_uniforms.append((type_, spelled, part[eq + 1:] if eq < len(part) else None))
            return ""
        if item.qualifiers & {"in", "out", "varying", "attribute"}:
            names = [self.text(part).strip() for (part, _) in parts]
            if any(t.is_op("[", "=") for t in tokens):
                # an array among them, which no fragment here has: the members as the array rewrite spells them, cut at the top-level
                # commas of that text (those of `sf_arr<T,n>` included) and joined again, which keeps such a fragment's text and cache key
                spelled = self.rewritten(tokens)
                at = _storage(spelled)[1]
                type_, names = spelled[at].text, [_text(run).strip() for run in _split_top_level(tokenize(_text(spelled[at + 1:-1])))]
            unknown = [n for n in names if n.split("[")[0].strip() not in BUILTIN_MEMBERS]
            return f"\n{type_} {', '.join(unknown)};" if unknown else ""
        if head == "struct":
            return self.struct(self.rewritten(tokens))
        if "const" in item.qualifiers and type_ in ("int", "float", "bool", "uint") and not any(t.is_op("[") for t in tokens):
            if all(self.literal(part[eq + 1:]) for (part, eq) in parts):
                for (part, eq) in parts:
                    name, value = part[_significant(part, 0)].text, [t.text for t in part[eq + 1:] if t.kind not in ("ws", "comment")]
                    self.constants.add(name)
                    if type_ == "int" and len(value) == 1 and value[0].isdigit():
                        self.constant_values[name] = int(value[0])
                return f"\nstatic constexpr {type_} {', '.join(self.text(part).strip() for (part, _) in parts)};"
        return self.text(tokens)

    def literal(self, tokens: list[Tok]) -> bool:
        """An initialiser that `static constexpr` can take: numbers, `true`, `false`, earlier such constants, `float`, `bool`, `int(` and
        `uint(`, and operators other than assignments, comparisons with `=`, `^^`, commas and brackets other than `()`"""
        words = [t for t in tokens if t.kind not in ("ws", "comment")]

        def passes(k: int, t: Tok) -> bool:
            if t.kind == "ident":
                return (t.text in self.constants or t.text in ("true", "false", "float", "bool") or set(t.text) <= _LITERAL_WORD
                        or (t.text in ("int", "uint") and k + 1 < len(words) and words[k + 1].is_op("(")))
            return t.kind == "number" or (t.kind == "op" and t.text != "^^" and set(t.text) <= _LITERAL_OPERATORS)
        return bool(words) and all(passes(k, t) for k, t in enumerate(words))

    def struct(self, tokens: list[Tok]) -> str:
        """`==` and `!=` of two structs compare member by member (§5.9): C++20 writes that comparison itself"""
        words = [k for k, t in enumerate(tokens) if t.kind not in ("ws", "comment")]
        open_ = next((k for k in words if tokens[k].is_op("{")), None)
        if open_ is None or len(words) < 3 or tokens[words[1]].kind != "ident" or words[2] != open_:
            return _text(tokens)
        close = _matching(tokens, open_, "{", "}")
        return _text(tokens[:close]) + f" SF_HD bool operator==(const {tokens[words[1]].text}&) const = default; " + _text(tokens[close:])

    def function(self, item: _Item) -> str:
        """A `#line` before the body (and after every directive inside it, which takes lines of its own here) keeps `__LINE__` (§3.3)
        and the compiler's messages on the lines of the GLSL text"""
        before = self.rewritten(item.tokens)
        return_type = next((t.text for t in before if t.kind == "ident"), "void")
        runs = [[t for t in self.rewritten(run) if t.kind not in ("ws", "comment")] for run in item.parameters]
        parameters = _rewrite_parameters(runs)
        head = ("\nSF_HD " + _text(before).lstrip() + "(" + ("" if parameters.strip() == "void" else parameters) + ")"
                + self.text(item.tail).rstrip() + f"\n#line {item.line}\n")
        body = self.function_body(self.rewritten(item.body), return_type, item.line)
        declared = [[t.text for t in run if t.text not in ("in", "out", "inout", "const")] for run in runs if run]
        samplers = [(position, words[1]) for position, words in enumerate(declared) if len(words) == 2 and words[0] == "sampler2D"]
        if samplers:                                               # for the tile heuristic: its taps are those of what a call passes
            first = sum(len(piece) for piece in self.body) + len(head)
            self.helpers.append((before[_significant(before, len(before) - 1, -1)].text, samplers, first + 1, first + len(body)))
        return head + body

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
        items = self.cut(raw)
        self.outs = out_parameters(items, _TYPES | self.structs)
        for item in items:
            if item.kind == "directive":
                self.body.append("\n" + self.preprocessor(item.tokens[0].text).strip("\n") + "\n")
            elif item.kind == "function":
                self.body.append(self.function(item))
            else:
                self.body.append(self.text(item.tokens) if item.kind == "text" else self.declaration(item))
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
        wanted = [(type_, [Tok("ident", name)], None) for (type_, name) in self.pipeline] + self.declared_uniforms
        declared_names = {_text(declarator).strip() for (_, declarator, _) in self.declared_uniforms}
        for (type_, declarator, default) in wanted:
            name = _text(declarator).strip()
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
            words = [t.text for t in declarator if t.kind != "ws"]
            word = lambda text: text.replace("_", "a").isalnum()       # a name or a whole number
            if len(words) == 4 and words[1::2] == ["[", "]"] and word(words[0]) and word(words[2]):
                name, length = words[0], self._array_length(words[2])
            elif "[" in name:
                raise TranslationError(f"uniform {name}: only one-dimensional arrays with a literal or constant size are supported")
            if type_ not in _UNIFORM_COUNTS:
                raise TranslationError(f"uniform {name}: type {type_} is not supported")
            count, integer = _UNIFORM_COUNTS[type_]
            if next_float + count*(length or 1) > USER_SLOTS:
                raise TranslationError(f"more than {USER_SLOTS} floats of uniforms")
            defaults = None
            if default and _significant(default, 0) < len(default):
                defaults = _constant_initialiser(type_, count, length, default, name)

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
        tiled = None if derivatives else _sampler_worth_a_tile(code, [b for b in bindings if b.type == "sampler2D"], self.helpers)
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


def _brackets(code: str, pair: str) -> tuple[list[int], list[Tok]]:
    """the brackets of `pair` in the emitted text, for _closing: their offsets, and they as operator tokens"""
    found = [(m.start(), Tok("op", m.group())) for m in re.finditer(f"[{re.escape(pair)}]", code)]
    return [at for at, _ in found], [t for _, t in found]


def _closing(code: str, brackets: tuple[list[int], list[Tok]], at: int) -> int:
    """index just past the bracket that closes the one at `at`, counting `brackets` alone; len(code) if none does"""
    offsets, tokens = brackets
    k = _scan(tokens, bisect.bisect_right(offsets, at), 1)
    return offsets[k] + 1 if k < len(offsets) else len(code)


def _loop_bodies(code: str, parentheses: tuple, braces: tuple) -> list[tuple[int, int]]:
    """(first, last) text ranges of the header and body of every for / while loop"""
    ranges = []
    for match in re.finditer(r"\b(?:for|while)\s*\(", code):
        header_end = _closing(code, parentheses, match.end() - 1)
        rest = code[header_end:]
        body = header_end + len(rest) - len(rest.lstrip())
        if body < len(code) and code[body] == "{":
            end = _closing(code, braces, body)
        else:
            semicolon = code.find(";", body)
            end = len(code) if semicolon < 0 else semicolon + 1
        ranges.append((match.start(), end))
    return ranges


def _sampler_worth_a_tile(code: str, samplers: list[Binding], helpers: list[tuple]) -> Optional[Binding]:
    """The sampler a tap-heavy fragment reads most (a blur or feedback kernel: taps inside the text of a loop, or eight and more
    written out), or None. SHADERFLOW_JIT_TILE=0 turns the tile off, =<sampler name> forces it for that sampler. `helpers`: the functions
    that take a sampler2D, (name, [(position, parameter)], first and last offset of the body in `code`).

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
    if not samplers:
        return None
    parentheses = _brackets(code, "()")
    loops = _loop_bodies(code, parentheses, _brackets(code, "{}"))
    in_loop = lambda at: any(first <= at < last for (first, last) in loops)
    weight = lambda at: 16 if in_loop(at) else 1
    tap_on = lambda names: re.compile(rf"\b{_TEXTURE_CALLS}\s*\(\s*(?:{'|'.join(map(re.escape, names))})\b")
    # helper functions that tap a sampler PARAMETER (`vec4 blur(sampler2D tex, vec2 uv) { for (…) … texture(tex, …) }`): the taps
    # count for whatever sampler a call passes in that position, once more heavily when the call itself sits in a loop
    tapping = []                                               # (name, position of the sampler parameter, weight of its taps, its calls)
    for (helper, parameters, first, last) in helpers:
        calls = [(call.start(), _split_top_level(tokenize(code[call.end():_closing(code, parentheses, call.end() - 1) - 1])))
                 for call in re.finditer(rf"\b{re.escape(helper)}\s*\(", code)]
        for (position, parameter) in parameters:
            taps = sum(weight(m.start()) for m in tap_on([parameter]).finditer(code, first, last))
            if taps:
                tapping.append((position, taps, calls))
    best, best_score = None, 0
    for binding in samplers:
        names = {binding.name, binding.name[:-3] if binding.name.endswith("0x0") else binding.name}
        score = sum(weight(m.start()) for m in tap_on(names).finditer(code))
        for (position, taps, calls) in tapping:
            for (at, arguments) in calls:
                if position < len(arguments) and _text(arguments[position]).strip() in names:
                    score += taps*weight(at)
        if score > best_score:
            best, best_score = binding, score
    return best if best_score >= 8 else None


def _constant_scalar(tokens: list[Tok], name: str) -> float:
    """A literal arithmetic expression of a uniform initialiser → its value (`-0.5`, `2.0*3.0`, `1e-3`, `true`, `3u`, `float(2)`).
    `int(…)` and `uint(…)` are conversions with results of their own here (to_int, to_uint) and no literals"""
    spelled = []
    for k, t in enumerate(tokens):
        nxt = _significant(tokens, k + 1)
        if t.kind == "comment":
            spelled.append("\n"*t.text.count("\n") or " ")
        elif t.kind == "ident" and t.text in ("true", "false"):
            spelled.append("1" if t.text == "true" else "0")
        elif t.kind == "ident" and t.text in ("float", "bool") and nxt < len(tokens) and tokens[nxt].is_op("("):
            spelled.append("")
        else:
            spelled.append(t.text)
    cleaned = re.sub(r"(?<=[0-9.])(?:lf|LF|[fFuU])\b", "", "".join(spelled).strip())
    try:
        tree = ast.parse(cleaned, mode="eval")
    except SyntaxError:
        raise TranslationError(f"uniform {name}: initialiser '{_text(tokens)}' is not a literal constant expression") from None
    allowed = (ast.Expression, ast.BinOp, ast.UnaryOp, ast.Constant, ast.Add, ast.Sub, ast.Mult, ast.Div, ast.USub, ast.UAdd)
    if not all(isinstance(node, allowed) for node in ast.walk(tree)):
        raise TranslationError(f"uniform {name}: initialiser '{_text(tokens)}' is not a literal constant expression")
    return float(eval(builtins.compile(tree, "<initialiser>", "eval"), {"__builtins__": {}}))      # (this module defines its own compile())


def _constant_value(type_: str, count: int, tokens: list[Tok], name: str) -> tuple:
    """`T(…)` or a scalar expression → `count` numbers (vector constructors splat a single argument, matrices put it on the diagonal)"""
    first, last = _significant(tokens, 0), _significant(tokens, len(tokens) - 1, -1)
    open_ = _significant(tokens, first + 1)
    constructor = open_ < last and tokens[first].text == type_ and type_ not in ("int", "uint") and tokens[open_].is_op("(") and tokens[last].is_op(")")
    if count == 1:
        return (_constant_scalar(tokens[open_ + 1:last] if constructor else tokens[first:last + 1], name),)
    if not constructor:
        raise TranslationError(f"uniform {name}: initialiser '{_text(tokens).strip()}' must be a {type_}(…) constructor of literals")
    arguments = [_constant_scalar(a, name) for a in _split_top_level(tokens[open_ + 1:last])]
    if len(arguments) == 1:
        if type_.startswith("mat"):
            side = int(type_[3])
            return tuple(arguments[0] if (k % (side + 1) == 0) else 0.0 for k in range(count))
        return tuple(arguments*count)
    if len(arguments) != count:
        raise TranslationError(f"uniform {name}: {type_} initialiser with {len(arguments)} components")
    return tuple(arguments)


def _constant_initialiser(type_: str, count: int, length: Optional[int], tokens: list[Tok], name: str) -> list[tuple]:
    """The initialiser of a uniform declaration as one tuple per element (one element for a non-array)"""
    if length is None:
        return [_constant_value(type_, count, tokens, name)]
    first, last = _significant(tokens, 0), _significant(tokens, len(tokens) - 1, -1)
    bracket = _significant(tokens, first + 1)
    constructor = tokens[first].text in _TYPES and bracket < last and tokens[bracket].is_op("[")         # `T[n](…)`, `T[](…)`
    open_ = _significant(tokens, _matching(tokens, bracket, "[", "]") + 1) if constructor else first       # … and a brace list is read as well
    if not (open_ < last and tokens[open_].is_op("(" if constructor else "{") and _scan(tokens, open_ + 1, 1) == last):
        raise TranslationError(f"uniform {name}: an array initialiser must be written {type_}[](…)")
    elements = _split_top_level(tokens[open_ + 1:last])
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
