"""CPU: the host's one statement of every kernel's parameter list (hamk_host.h, namespace sig) against the device headers.
launch_kernel<Sig> builds a launch's argument array from that table, so a type or an order that differs from the kernel's own is a kernel
reading garbage: here every `extern "C" __global__ ... name(params)` of the five device headers is reduced to its list of parameter
types, the three HAMK_INSTANTIATE* macros must agree on the eight kernels of the path, and every kernel must equal the table's entry.
Text only: nothing is compiled."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hamilton_amd", "csrc")
PATH_KERNELS = ["hamk_rk4_steps_k", "hamk_hameqs_k", "hamk_coords_k", "hamk_to_phase_k", "hamk_from_phase_k", "hamk_observe_k",
                "hamk_observe_config_k", "hamk_rkf45_k"]
ALL_KERNELS = PATH_KERNELS + ["hamk_scribble_k", "hamk_symp_steps_k", "hamk_sample_k"]


def _text(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read().replace("\\\n", "\n")                    # macro bodies: line continuations are layout


def _types(params, named):
    """`const double* q, long long B` -> ['const double*', 'long long'] (named: the trailing identifier of each parameter goes)."""
    out = []
    for p in params.split(","):
        p = " ".join(p.split())
        if named:
            p = re.sub(r"\s*\b[A-Za-z_]\w*$", "", p)
        out.append(re.sub(r"\s*\*", "*", p))
    return out


def device_kernels(header):
    """name -> parameter types, for every kernel DEFINITION of the header (HIP builds; the host-emulation stub of hamk_scribble_k is no kernel)."""
    found = {}
    for m in re.finditer(r'extern "C" __global__ void\s+(?:__launch_bounds__\([^{;]*?\)\s+|HAMK_\w+BOUNDS\w*\s+)?(hamk_\w+_k)\s*\(([^)]*)\)\s*\{', _text(header)):
        assert m.group(1) not in found, f"{header}: {m.group(1)} twice"
        found[m.group(1)] = _types(m.group(2), named=True)
    return found


def host_table():
    body = re.search(r"namespace sig \{(.*?)\}  // namespace sig", _text("hamk_host.h"), re.S).group(1)
    return {m.group(1): _types(m.group(2), named=False) for m in re.finditer(r"using (hamk_\w+_k) = void\(([^)]*)\);", body)}


def test_the_parser_reads_a_known_kernel():
    assert device_kernels("hamk_device.hpp")["hamk_coords_k"] == ["const double*", "double*", "long long"]
    assert device_kernels("hamk_sample.hpp")["hamk_sample_k"][-1] == "HamkBoxes"


def test_the_three_mappings_state_the_same_eight_kernels():
    lane, quad, wave = (device_kernels(h) for h in ("hamk_device.hpp", "hamk_quad.hpp", "hamk_wave.hpp"))
    assert sorted(quad) == sorted(PATH_KERNELS) and sorted(wave) == sorted(PATH_KERNELS)
    assert sorted(lane) == sorted(PATH_KERNELS + ["hamk_scribble_k"])
    for k in PATH_KERNELS:
        assert lane[k] == quad[k] == wave[k], k


def test_every_kernel_equals_the_host_table():
    host = host_table()
    assert sorted(host) == sorted(ALL_KERNELS)
    device = {}
    for h in ("hamk_device.hpp", "hamk_quad.hpp", "hamk_wave.hpp", "hamk_symp.hpp", "hamk_sample.hpp"):
        for k, types in device_kernels(h).items():
            assert types == host[k], (h, k)
            device[k] = types
    assert sorted(device) == sorted(ALL_KERNELS)
