"""tests/golden/tonemap_table.npz: the reference's own tonemap (libs/yocto/yocto_color.h:306-316) and float_to_byte (:207-211) over
about a thousand float4 inputs, for every display setting the tests use.  Run where the reference's sources lie:

    python tests/golden/make_tonemap_fixture.py <reference root>        (or REF=<reference root> in the environment)

The script writes a few lines of C++ of its own into a temporary directory; they include the reference's header-only
yocto/yocto_color.h in place (g++ -std=c++17 -I<reference>/libs -ffp-contract=off, x86-64 baseline as oracle/Makefile: no fused
operations), read the inputs from a file and write the outputs to another.  Neither the program nor any reference text is kept.

Inputs (1024 float4, float32): log-uniform values from 1e-6 to 1e3, the values 0, 0.0031308f and its
float neighbours, 1 and its neighbours, small negatives, a few exact quantisation steps k / 256.  Every a * 256 that float_to_byte
converts stays far inside the int range for every setting (|a| <= 1e3 * 2^1.25 * 256 < 2^20), and every value is finite: int(a * 256)
is defined in the reference for all of them.
Settings: exposure in {0, -2.5, 1.25} x filmic in {0, 1} x srgb in {0, 1}, in that order (exposure outermost).
Arrays: inputs (n, 4) float32; settings (12, 3) float32 {exposure, filmic, srgb}; floats (12, n, 4) float32; bytes (12, n, 4) uint8."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <yocto/yocto_color.h>
using namespace yocto;
int main(int argc, char** argv) {
  auto n = atoi(argv[1]);
  auto exposure = (float)atof(argv[2]);
  auto filmic = atoi(argv[3]) != 0, srgb = atoi(argv[4]) != 0;
  auto in = std::vector<vec4f>(n);
  auto f = fopen(argv[5], "rb");
  if (!f || fread(in.data(), sizeof(vec4f), n, f) != (size_t)n) return 1;
  fclose(f);
  auto outf = std::vector<vec4f>(n);
  auto outb = std::vector<vec4b>(n);
  for (auto i = 0; i < n; i++) {
    outf[i] = tonemap(in[i], exposure, filmic, srgb);
    outb[i] = float_to_byte(outf[i]);
  }
  f = fopen(argv[6], "wb");
  if (!f || fwrite(outf.data(), sizeof(vec4f), n, f) != (size_t)n || fwrite(outb.data(), sizeof(vec4b), n, f) != (size_t)n) return 1;
  fclose(f);
  return 0;
}
"""

EXPOSURES, FLAGS = (0.0, -2.5, 1.25), (0, 1)


def make_inputs():
    rng = np.random.default_rng(20240611)
    F = np.float32
    knee, one = F(0.0031308), F(1)
    special = [F(0), knee, np.nextafter(knee, F(0)), np.nextafter(knee, F(1)), one, np.nextafter(one, F(0)), np.nextafter(one, F(2)),
               F(-1e-6), F(-1e-3), F(-0.25), F(0.18), F(0.5)] + [F(k / 256) for k in (1, 2, 127, 128, 254, 255, 256)]
    values = np.concatenate([np.array(special, F), np.exp(rng.uniform(np.log(1e-6), np.log(1e3), 4 * 1024 - len(special))).astype(F)])
    rng.shuffle(values)
    return np.ascontiguousarray(values.reshape(1024, 4))


def main():
    ref = (sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF", ""))
    if not os.path.exists(os.path.join(ref, "libs", "yocto", "yocto_color.h")):
        sys.exit("usage: make_tonemap_fixture.py <reference root>   (no libs/yocto/yocto_color.h under %r)" % ref)
    inputs = make_inputs()
    n = len(inputs)
    settings, floats, bytes_ = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "table.cpp"), os.path.join(tmp, "table")
        open(src, "w").write(PROGRAM)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ref, "libs"), src, "-o", exe])
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        inputs.tofile(fin)
        for exposure in EXPOSURES:
            for filmic in FLAGS:
                for srgb in FLAGS:
                    subprocess.check_call([exe, str(n), repr(exposure), str(filmic), str(srgb), fin, fout])
                    raw = open(fout, "rb").read()
                    floats.append(np.frombuffer(raw, np.float32, n * 4).reshape(n, 4))
                    bytes_.append(np.frombuffer(raw, np.uint8, n * 4, n * 16).reshape(n, 4))
                    settings.append((exposure, filmic, srgb))
    out = os.path.join(HERE, "tonemap_table.npz")
    np.savez_compressed(out, inputs=inputs, settings=np.array(settings, np.float32), floats=np.array(floats), bytes=np.array(bytes_))
    print("wrote", out, os.path.getsize(out), "bytes;", len(settings), "settings x", n, "pixels")


if __name__ == "__main__":
    main()
