#!/usr/bin/env python3
"""Rewrite the reference's compute shader into text a C++20 compiler accepts beside
oracle/glsl_shim.h. Build-time only: reads <reference>/shaders, writes <out>/ (oracle/_ref/shader,
git-ignored). Nothing of the shader is kept here: the rules below name only the GLSL keywords
and identifiers they replace.

Every rule is (file, pattern, replacement, exact number of lines it must hit). Any other count
fails the build, so drift in the reference is noticed. A rule works inside one line and the line
count never changes; after the rules the output is compared with the input again and may differ
on the rules' lines only. No rule touches an arithmetic expression, a literal, an operand order
or control flow (DESIGN.md section 3 lists them).
"""
import os
import re
import sys

FILES = ("shader.comp", "include/functions.glsl", "include/globals.glsl",
         "include/structures.glsl", "include/textures.glsl")

COMP, FUNC, GLOB, STRUCT, TEX = FILES

RULES = [
    # 1. declarations only a GLSL front end reads
    (COMP, r"^#version .*$", "", 1),
    (COMP, r"^#extension .*$", "", 1),
    (COMP, r"^layout *\(.*;$", "", 2),
    (STRUCT, r"^precision \w+ float;$", "", 1),
    # 2. parameter qualifiers -> references (inout, out) or nothing (in)
    (FUNC, r"\binout (\w+) (\w+)", r"\1& \2", 1),
    (TEX, r"\binout (\w+) (\w+)", r"\1& \2", 4),
    (FUNC, r"(?<![a-z])out (\w+) (\w+)", r"\1& \2", 1),
    (TEX, r"(?<![a-z])out (\w+) (\w+)", r"\1& \2", 1),
    (FUNC, r"\bconst in\b", "const", 1),
    (TEX, r"\bconst in\b", "const", 1),
    # 3. the array's length -> a shim name
    (FUNC, r"\bworld\.length\(\)", "ref_world_length()", 1),
    # 4. the entry point -> a named function
    (COMP, r"^void main\(\)", "void ref_shader_main()", 1),
    # 5. compile-time configuration -> run-time ints (IMAGE_WIDTH/IMAGE_HEIGHT stays an
    #    integer division)
    (GLOB, r"^#define (SAMPLES_PER_PIXEL) (\d+)$", r"int \1 = \2;", 2),
    (GLOB, r"^#define (MAX_RECURSION_LEVEL) (\d+)$", r"int \1 = \2;", 1),
    (GLOB, r"^#define (IMAGE_WIDTH) (\d+)$", r"int \1 = \2;", 1),
    (GLOB, r"^#define (IMAGE_HEIGHT) (\d+)$", r"int \1 = \2;", 1),
    # 6. the scene array renamed: `world` is the shim's run-time view, this its default
    (GLOB, r"^const sphere world\[\] =", "const sphere ref_world_default[] =", 1),
]
# 7. ray_color is the last function of functions.glsl and flows off its end (undefined in GLSL
#    and in C++): its closing brace, the file's last line, gets the canonical return in front.
LAST_BRACE = (FUNC, r"^\}$", "return ref_undefined_return(); }", "ray_color")


def fail(msg):
    sys.exit(f"glsl_rewrite: {msg}")


def rewrite(src_dir, out_dir):
    texts = {}
    for f in FILES:
        with open(os.path.join(src_dir, f), encoding="utf-8") as fh:
            texts[f] = fh.read().split("\n")
    out = {f: list(lines) for f, lines in texts.items()}
    touched = {f: set() for f in FILES}

    for f, pat, rep, want in RULES:
        rx = re.compile(pat)
        hits = 0
        for i, line in enumerate(out[f]):
            new, n = rx.subn(rep, line.rstrip("\r"))
            if n:
                hits += 1
                out[f][i] = new
                touched[f].add(i)
        if hits != want:
            fail(f"rule {pat!r} hit {hits} lines of {f}, expected {want}: the reference changed")

    f, pat, rep, fn = LAST_BRACE
    lines = out[f]
    last = max(i for i, line in enumerate(lines) if line.strip())
    if not re.match(pat, lines[last].rstrip("\r")):
        fail(f"{f} does not end with a closing brace")
    headers = [i for i, line in enumerate(lines) if re.match(r"^\w+ \w+\(.*\) *\{\s*$", line)]
    if not headers or not re.match(rf"^vec3 {fn}\(", lines[headers[-1]]):
        fail(f"the last function of {f} is not {fn}")
    lines[last] = rep
    touched[f].add(last)

    for f in FILES:  # the output differs from the input on the rules' lines only
        with open(os.path.join(src_dir, f), encoding="utf-8") as fh:
            again = fh.read().split("\n")
        if len(again) != len(out[f]):
            fail(f"{f}: line count changed")
        for i, (a, b) in enumerate(zip(again, out[f])):
            if a != b and i not in touched[f]:
                fail(f"{f}:{i + 1} changed outside a rule")
            if a.rstrip("\r") == b and i in touched[f] and a.strip():
                fail(f"{f}:{i + 1} hit by a rule but unchanged")

    for f in FILES:
        path = os.path.join(out_dir, f)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w", encoding="utf-8") as fh:
            fh.write("\n".join(out[f]))


if __name__ == "__main__":
    if len(sys.argv) != 3:
        fail("usage: glsl_rewrite.py <reference>/shaders <out dir>")
    rewrite(sys.argv[1], sys.argv[2])
