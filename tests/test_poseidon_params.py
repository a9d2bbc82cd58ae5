"""CPU: the C++ Grain generator of the Poseidon parameters (sylow_amd/csrc/poseidon_params.hpp) against the Python model, which shares no
code with it.  The header compiles alone with g++; a stand-alone program (tests/cpp/poseidon_params_main.cpp), built under the address and
undefined-behaviour sanitizers, prints the round constants and the sums xs[i] + ys[j] of every width t = 2 .. 17, and every line is compared.
Host code only: nothing here is loaded into Python."""
import os
import subprocess

import poseidon_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "sylow_amd", "csrc", "poseidon_params.hpp")


def test_the_header_compiles_alone(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { return poseidon_params::rounds(3) == 65 ? 0 : 1; }\n' % HEADER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-o", str(tmp_path / "alone.o")], check=True, timeout=300)
    text = open(HEADER).read()
    assert '#include "' not in text, "no include of the project's"


def test_the_cpp_generator_draws_what_the_model_draws(tmp_path):
    exe = str(tmp_path / "poseidon_params_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "poseidon_params_main.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = {}
    for line in r.stdout.split("\n"):
        if line:
            tag, t, i, v = line.split()
            got.setdefault((tag, int(t)), []).append(int(v, 16))
            assert int(i) == len(got[tag, int(t)]) - 1
    assert sorted(got) == sorted((tag, t) for tag in "CS" for t in range(2, 18))
    for t in range(2, 18):
        consts, xs, ys = P.draws(t)
        assert got["C", t] == list(consts), t
        assert got["S", t] == [(x + y) % P.R for x in xs for y in ys], t
