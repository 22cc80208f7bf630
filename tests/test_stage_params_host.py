"""The parameter table every object behind the backbone declares (csrc/rn_params.h), without a GPU: a stand-alone
program under the host sanitizers, nothing of it is loaded into this process.  examples/params_check.cpp declares the
tables of a 2-level neck, an RPN, a box head and a 2-layer mask head as their create functions do and checks: every
key and every other spelling to its slot, the optional prefix, unknown keys, a wrong numel (given and wanted apart),
set twice (the second values are written out; the leak check of the sanitizer stays quiet), first-missing, the padded
write-out with its fill, and a full table refusing one more entry."""
import os
import subprocess


def test_parameter_table_under_the_host_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "params_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",   # the runtimes inside the program
                    f"-I{root}/resnet.c_amd/csrc", f"{root}/examples/params_check.cpp", "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "every expectation holds" in r.stdout, r.stdout + r.stderr
