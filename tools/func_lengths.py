"""Longest host functions of the CLI (metamaps_amd/csrc/host/) and of the library (metamaps_amd/csrc/*.hip): none above 200 lines (round-4 review item 8,
round-6 item 8); and of the device allocator's headers (mm_alloc.hpp, mm_alloc_rules.hpp, mm_stream.hpp): none above 60.  A function = a brace block whose opening line ends in ') {' or ') const {' (or carries a trailing comment behind that); methods of structs count.
Device code is left out: a function whose declaration carries __global__ or __device__, on the opening line or on the earlier lines of a multi-line signature
(back to the previous ';', '}' or blank line).  Kernels are judged by other means.
The line before them lists the library's .hip files in which host functions were found.
The line before the last names the longest file of metamaps_amd/csrc/host/: none above 800 lines (the CLI was one file of 2 488; map_run.hpp stood at 999
by squeezing its lines), and the line before that the longest line of those files: none above 200 characters."""
import glob, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_decl(lines, i):
    while True:
        if "__global__" in lines[i] or "__device__" in lines[i]:
            return True
        i -= 1
        if i < 0 or not lines[i].strip() or lines[i].split("//")[0].rstrip().endswith((";", "}")):
            return False


def functions(path):
    lines = open(path).read().split("\n")
    depth, stack, out = 0, [], []
    for i, ln in enumerate(lines):
        code = re.sub(r'"(?:[^"\\]|\\.)*"', '""', ln)
        code = re.sub(r"'(?:[^'\\]|\\.)'", "''", code).split("//")[0]
        opens, closes = code.count("{"), code.count("}")
        if opens > closes and not device_decl(lines, i) and re.search(r"\)\s*(const\s*)?(noexcept\s*)?(->\s*[\w:<>]+\s*)?\{\s*$", code.rstrip()) and not re.match(r"\s*(if|for|while|switch|else|do)\b", code) and "[&" not in code and "[=" not in code and "[this" not in code:
            stack.append((depth, i, ln.strip()[:90]))
        depth += opens - closes
        while stack and depth <= stack[-1][0]:
            d0, i0, name = stack.pop()
            out.append((i - i0 + 1, os.path.relpath(path, ROOT), i0 + 1, name))
    return out


if __name__ == "__main__":
    csrc = os.path.join(ROOT, "metamaps_amd", "csrc")
    host = [fn for f in sorted(glob.glob(os.path.join(csrc, "host", "*"))) for fn in functions(f)]
    lib = [fn for f in sorted(glob.glob(os.path.join(csrc, "*.hip"))) for fn in functions(f)]
    alloc = sorted((fn for f in ("mm_alloc.hpp", "mm_alloc_rules.hpp", "mm_stream.hpp") for fn in functions(os.path.join(csrc, f))), reverse=True)
    allf = sorted(host + lib, reverse=True)
    for n, f, l, name in allf[:12] + alloc[:3]:
        print(f"{n:5d}  {f}:{l}  {name}")
    files = sorted((len(open(f).read().split("\n")) - 1, os.path.relpath(f, ROOT)) for f in glob.glob(os.path.join(csrc, "host", "*")))
    wide = max((len(ln), os.path.relpath(f, ROOT), i + 1) for f in glob.glob(os.path.join(csrc, "host", "*")) for i, ln in enumerate(open(f).read().split("\n")))
    print("library files: " + " ".join(sorted({os.path.basename(f) for _, f, _, _ in lib})))   # (every csrc/*.hip in which a host function was found)
    print(f"longest line: {wide[0]} {wide[1]}:{wide[2]}")
    print(f"longest file: {files[-1][0]} {files[-1][1]} of {len(files)} csrc/host")
    print(f"functions: {len(host)} csrc/host {len(lib)} csrc/*.hip {len(alloc)} csrc/mm_alloc.hpp+mm_alloc_rules.hpp+mm_stream.hpp")
    sys.exit(1 if (allf and allf[0][0] > 200) or (alloc and alloc[0][0] > 60) or files[-1][0] > 800 or wide[0] > 200 else 0)
