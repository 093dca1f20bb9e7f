"""ctypes binding of the C-ABI in include/mobocmf_hip.h (libmobocmf_hip.so, built by csrc/build.sh).

The header is the only statement of that ABI: the constants, the struct layouts and every entry point's argument types are
read from it once, at import (_header.py).  What the header does not say is written here, and nothing else.

The product path has NO CPU fallback: if the shared library is missing or the device is not a
gfx950, every compute entry point raises.
"""
import ctypes
import os

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MOBOCMF_HIP_LIB") or os.path.join(_HERE, "csrc", "libmobocmf_hip.so")   # override: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mobocmf_hip.h")      # A/B libraries share the tree's header


class MobocmfError(RuntimeError):
    pass


def read_header(path):
    try:
        with open(path) as f:
            return _header.Header(f.read())
    except OSError as e:
        raise MobocmfError(f"C header missing: {path} ({e.strerror}); the ctypes binding is derived from it") from e


_ABI = read_header(HEADER_PATH)
CONSTANTS = _ABI.constants          # every MOBOCMF_X of the header, enum included, as X
globals().update(CONSTANTS)         # OK, BAD_ARG, ..., MAX_D, TINY_MAX_M, STEP_UPDATE, EXACT_FIT_W_IT, ...
_ERR = {CONSTANTS[name]: "MOBOCMF_" + name for name in _ABI.enum}
STRUCTS = {}                        # C name -> class
SYMBOLS = _ABI.functions            # name -> argtypes   (every symbol include/mobocmf_hip.h declares)
_SZ = ctypes.c_size_t


def _struct(c_name):
    """Class decorator: the class takes the fields of the header's struct c_name."""
    def bind(cls):
        cls._fields_ = _ABI.fields(c_name, STRUCTS)
        STRUCTS[c_name] = cls
        return cls
    return bind


def _knobs(cls, first):
    return tuple(n for n, _ in cls._fields_[first:])


@_struct("mobocmf_tuning")
class Tuning(ctypes.Structure):
    """The kernel-selection knobs that travel with a call (NULL = defaults)."""

    def copy(self):
        t = Tuning()
        ctypes.memmove(ctypes.byref(t), ctypes.byref(self), ctypes.sizeof(Tuning))
        return t


@_struct("mobocmf_layer_desc")
class LayerDesc(ctypes.Structure):
    pass


@_struct("mobocmf_rff_layer_desc")
class RffLayerDesc(ctypes.Structure):
    """One layer of one chain sample of mobocmf_rff_eval_chains (the kernel reads the table from DEVICE memory)."""


@_struct("mobocmf_rff_refine_options")
class RffRefineOptions(ctypes.Structure):
    """The settings of mobocmf_rff_refine, passed with the call (NULL = defaults)."""


@_struct("mobocmf_nsga_options")
class NsgaOptions(ctypes.Structure):
    """The settings of mobocmf_nsga_vary, passed with the call (NULL = defaults)."""


@_struct("mobocmf_tiny_model")
class TinyModel(ctypes.Structure):
    """One small surrogate of mobocmf_tiny_elbo_step (the kernel reads the array from DEVICE memory)."""


@_struct("mobocmf_tiny_coupling")
class TinyCoupling(ctypes.Structure):
    """The theta / omega factors over the models of one mode-4 launch (device-resident)."""


@_struct("mobocmf_natgrad_small_layer")
class NatgradSmallLayer(ctypes.Structure):
    """One layer of mobocmf_natgrad_small_step (the kernel reads the array from DEVICE memory)."""


@_struct("mobocmf_frozen_predict_model")
class FrozenPredictModel(ctypes.Structure):
    """One surrogate of mobocmf_frozen_predict[_split] (the kernel reads the array from DEVICE memory)."""


@_struct("mobocmf_exact_predict_model")
class ExactPredictModel(ctypes.Structure):
    """One exact-GP surrogate of mobocmf_exact_predict (the kernel reads the array from DEVICE memory)."""


@_struct("mobocmf_exact_fit_param")
class ExactFitParam(ctypes.Structure):
    """One raw parameter tensor of a model of the device fit, its constraint and its optimiser state."""


@_struct("mobocmf_exact_fit_model")
class ExactFitModel(ctypes.Structure):
    """One exact-GP surrogate of the mobocmf_exact_fit_* launches (read from DEVICE memory)."""


@_struct("mobocmf_exact_sample_problem")
class ExactSampleProblem(ctypes.Structure):
    """One (model, sample) of the mobocmf_exact_sample_* launches (read from DEVICE memory)."""


Tuning.KNOBS, RffRefineOptions.KNOBS, NsgaOptions.KNOBS = _knobs(Tuning, 1), _knobs(RffRefineOptions, 1), _knobs(NsgaOptions, 2)

# ---- what the header states in prose only
NATGRAD_MAX_LAYERS = 4            # layers per mobocmf_natgrad_step call
# positions of the sums in the slab of the device fit (MOBOCMF_EXACT_FIT_SUMS of them)
EXACT_FIT_S_OS_S, EXACT_FIT_S_LS_S, EXACT_FIT_S_OS_N, EXACT_FIT_S_LS_N, EXACT_FIT_S_TAU, EXACT_FIT_S_SIG, EXACT_FIT_S_NTAB = \
    0, 1, 33, 34, 66, 67, 75
HV_MAX_POINTS = {1: 65536, 2: 65536, 3: 65536, 4: 1024, 5: 256}   # the work bound of mobocmf_hypervolume
REFINE_STATUS = {0: "refinement moved away from the best start", 1: "the best start itself is returned",
                 2: "no start has a feasible result"}            # status of mobocmf_rff_refine
INDUCING_INFO = {1: "a non-finite entry of x", 2: "a non-finite or non-positive hyper-parameter"}   # info of mobocmf_select_inducing
MINIBATCH_STATUS = {                                              # status word of mobocmf_minibatch_indices
    CONSTANTS["MINIBATCH_ROWS_MISMATCH"]: "the batch does not have the rows the step was built for (host and device step "
                                          "counts differ)",
    CONSTANTS["MINIBATCH_BAD_STATE"]: "a negative step count"}

_lib = None


def load():
    """Loads the shared library (no GPU needed for loading / symbol checks)."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  -- first: the HIP runtime torch ships must be the one this library binds to
        if not os.path.exists(LIB_PATH):
            raise MobocmfError(f"HIP extension missing: {LIB_PATH} (run mobocmf_amd/csrc/build.sh or "
                               "__graft_entry__.build()); there is no CPU fallback")
        lib = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SYMBOLS.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int
        _lib = lib
    return _lib


def check(rc, what):
    if rc != CONSTANTS["OK"]:
        raise MobocmfError(f"{what} failed: {_ERR.get(rc, rc)}")


_arch_checked = False


def require_device():
    """Fail loudly unless a gfx950 device is current."""
    global _arch_checked
    lib = load()
    if not _arch_checked:
        import torch
        if not torch.cuda.is_available():
            raise MobocmfError("mobocmf_amd needs an MI355X (gfx950) device: no GPU visible, and there is no CPU fallback")
        if not lib.mobocmf_device_arch_ok():
            raise MobocmfError("mobocmf_amd kernels are built for gfx950 only")
        _arch_checked = True
    return lib
