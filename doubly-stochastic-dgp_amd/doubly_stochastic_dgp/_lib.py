"""ctypes binding of libdsdgp.so (include/dsdgp.h).  There is NO CPU fallback: if the HIP library is missing or no
MI355X is visible, importing the compute path raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSDGP_LIB_PATH: development override (A/B builds of the kernels); the shipped library is csrc/libdsdgp.so
_LIB_PATH = os.environ.get("DSDGP_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "csrc", "libdsdgp.so")

DSDGP_MAX_LAYERS = 16
KERN_RBF, KERN_MATERN52 = 0, 1
MEAN_ZERO, MEAN_IDENTITY, MEAN_LINEAR = 0, 1, 2
LIK_GAUSSIAN, LIK_MULTICLASS, LIK_BERNOULLI, LIK_POISSON, LIK_EXPONENTIAL, LIK_STUDENT_T, LIK_GAMMA, LIK_BETA = 0, 1, 2, 3, 4, 5, 6, 7
ERR_NOT_SPD = -2
ERR_UNSUPPORTED = -4
MAT_LU, MAT_LUINV, MAT_LUINVT, MAT_KUINV = 0, 1, 2, 3
ERR_RCCL = -6

c_double_p = C.POINTER(C.c_double)


class DsdgpError(RuntimeError):
    pass


class CholeskyError(DsdgpError):
    """mirrors TF's InvalidArgumentError 'Cholesky decomposition was not successful' (layers.py:172)"""


class KernelSpec(C.Structure):
    _fields_ = [("kind", C.c_int32), ("input_dim", C.c_int32), ("ard", C.c_int32), ("has_white", C.c_int32),
                ("variance", C.c_double), ("white_variance", C.c_double), ("lengthscales", c_double_p)]


class LayerDesc(C.Structure):
    _fields_ = [("M", C.c_int32), ("D_in", C.c_int32), ("D_out", C.c_int32),
                ("kern_kind", C.c_int32), ("ard", C.c_int32), ("has_white", C.c_int32),
                ("mean_kind", C.c_int32),
                ("trainable_Z", C.c_int32), ("trainable_q_mu", C.c_int32), ("trainable_q_sqrt", C.c_int32),
                ("trainable_kvar", C.c_int32), ("trainable_kls", C.c_int32), ("trainable_wvar", C.c_int32),
                ("input_prop_dim", C.c_int32),
                ("trainable_mean_A", C.c_int32), ("trainable_mean_b", C.c_int32),
                ("kvar_identity", C.c_int32), ("reserved0", C.c_int32),
                ("mean_A", C.c_void_p),
                ("off_Z", C.c_int64), ("off_q_mu", C.c_int64), ("off_q_sqrt", C.c_int64),
                ("off_kvar", C.c_int64), ("off_kls", C.c_int64), ("off_wvar", C.c_int64),
                ("off_mean_A", C.c_int64), ("off_mean_b", C.c_int64)]


class ModelDesc(C.Structure):
    _fields_ = [("L", C.c_int32), ("white", C.c_int32), ("lik_kind", C.c_int32), ("num_classes", C.c_int32),
                ("trainable_lik_var", C.c_int32), ("reserved", C.c_int32),
                ("jitter", C.c_double), ("lik_aux", C.c_double), ("off_lik_var", C.c_int64), ("n_theta", C.c_int64),
                ("layers", LayerDesc * DSDGP_MAX_LAYERS)]


class StackLayer(C.Structure):
    """dsdgp_stack_layer: Z, q_mu, mean_A, mean_b are device pointers"""
    _fields_ = [("kern", KernelSpec), ("Z", C.c_void_p), ("q_mu", C.c_void_p), ("mean_A", C.c_void_p), ("mean_b", C.c_void_p),
                ("M", C.c_int32), ("DO", C.c_int32), ("white", C.c_int32), ("mean_kind", C.c_int32), ("input_prop_dim", C.c_int32),
                ("reserved", C.c_int32)]


class StackDesc(C.Structure):
    """dsdgp_stack_desc"""
    _fields_ = [("L", C.c_int32), ("lik_kind", C.c_int32), ("lik_width", C.c_int32), ("reserved", C.c_int32),
                ("lik_p0", C.c_double), ("lik_p1", C.c_double), ("jitter", C.c_double), ("layers", StackLayer * DSDGP_MAX_LAYERS)]


_lib = None

_PROTOS = {
    "dsdgp_version": (C.c_int, []),
    "dsdgp_sizeof_layer_desc": (C.c_int, []),
    "dsdgp_sizeof_model_desc": (C.c_int, []),
    "dsdgp_last_error": (C.c_char_p, []),
    "dsdgp_ctx_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    "dsdgp_ctx_destroy": (C.c_int, [C.c_void_p]),
    "dsdgp_sync": (C.c_int, [C.c_void_p]),
    "dsdgp_prof_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "dsdgp_prof_read": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
    "dsdgp_launch_count": (C.c_int64, []),
    "dsdgp_gram": (C.c_int, [C.c_void_p, C.POINTER(KernelSpec), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                             C.c_double, C.c_void_p, C.c_int64]),
    "dsdgp_potrf": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_int)]),
    "dsdgp_trsm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "dsdgp_trsm_batched": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                     C.c_int64, C.c_int64]),
    "dsdgp_gemm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p,
                             C.c_int64, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_int64]),
    "dsdgp_model_workspace_bytes": (C.c_int, [C.POINTER(ModelDesc), C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "dsdgp_model_create": (C.c_int, [C.c_void_p, C.POINTER(ModelDesc), C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]),
    "dsdgp_model_destroy": (C.c_int, [C.c_void_p]),
    "dsdgp_model_prepare": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "dsdgp_model_propagate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_int64), C.c_uint64, C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "dsdgp_model_elbo": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_int64), C.c_uint64, C.c_double, C.c_double, C.c_int, C.c_void_p]),
    "dsdgp_model_forward_saved": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                            C.c_uint64, C.c_void_p, C.c_void_p]),
    "dsdgp_model_backward_adjoints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    "dsdgp_model_adam_step": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64]),
    "dsdgp_model_train_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_int64), C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double,
                                         C.c_double, C.c_double, C.c_int64, C.c_void_p]),
    "dsdgp_model_train_step_minibatch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                                   C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                                   C.c_int64, C.c_void_p]),
    "dsdgp_model_set_bucket_callback": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "dsdgp_model_set_sample_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "dsdgp_model_natgrad_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.POINTER(C.c_int)]),
    "dsdgp_model_layer_kl": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "dsdgp_model_layer_matrix": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]),
    "dsdgp_model_layer_conditional": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "dsdgp_model_layer_conditional_full": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "dsdgp_reparameterize_full": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int64, C.c_int32,
                                            C.c_int32, C.c_void_p]),
    "dsdgp_reparameterize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int64, C.c_void_p]),
    "dsdgp_randn": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p]),
    "dsdgp_gather_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "dsdgp_gather_rows2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_int64, C.c_int64]),
    "dsdgp_gauss_var_exp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                      C.c_double, C.c_void_p, C.c_void_p]),
    "dsdgp_gauss_predict_density": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                              C.c_int32, C.c_double, C.c_void_p]),
    "dsdgp_add_scalar": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_int64, C.c_void_p]),
    "dsdgp_multiclass_var_exp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                           C.c_int, C.c_void_p, C.c_void_p]),
    "dsdgp_multiclass_predict": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "dsdgp_bernoulli_var_exp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                          C.c_int, C.c_void_p, C.c_void_p]),
    "dsdgp_bernoulli_predict": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "dsdgp_lik_var_exp": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p]),
    "dsdgp_lik_predict": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_void_p]),
    "dsdgp_lik_elbo_readout": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int64]),
    "dsdgp_multiclass_readout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_double,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dsdgp_eval_mixture": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]),
    "dsdgp_model_evaluate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_int64), C.c_uint64, C.c_void_p, C.c_void_p, C.c_int]),
    "dsdgp_mixture_quantiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int64, C.c_int32, C.c_int32, c_double_p,
                                          C.c_int32, C.c_void_p]),
    "dsdgp_mixture_calibration": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                            c_double_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]),
    "dsdgp_model_quantiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                        C.c_uint64, C.c_int32, c_double_p, C.c_int32, C.c_void_p]),
    "dsdgp_model_calibration": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_int64), C.c_uint64, c_double_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]),
    "dsdgp_mixture_classification": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                               C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "dsdgp_model_classification": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_int64), C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "dsdgp_kmeans": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p]),
    "dsdgp_greedy_inducing": (C.c_int, [C.c_void_p, C.POINTER(KernelSpec), C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_double,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "dsdgp_pca": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # layers.py:415-417, 494-495: expectation(DiagonalGaussian, (RBF, InducingPoints)[, (RBF, InducingPoints)])
    "dsdgp_rbf_expectations": (C.c_int, [C.c_void_p, C.POINTER(KernelSpec), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    # the reverse pass tf.gradients builds through layers.py:415-417 (tests/test_collapsed.py:10, tests/test_dgp.py:150: ScipyOptimizer().minimize(m))
    "dsdgp_rbf_expectations_grad": (C.c_int, [C.c_void_p, C.POINTER(KernelSpec), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_int64, C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    # layers.py:426-427 (tf.transpose(tmp), AAT / sigma2, AAT + eye), :443-448 (the bound's terms), :521-524 (the predictive variance)
    "dsdgp_scale_copy": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p,
                                   C.c_int64]),
    "dsdgp_collapsed_bound": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    "dsdgp_collapsed_var": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                      C.c_double, C.c_void_p]),
    "dsdgp_collapsed_adjoints": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    # the reverse pass tf.gradients builds through kern.K of the dense layers (layers.py:278-279, 320-342; model_zoo.py:60-88)
    "dsdgp_gram_grad": (C.c_int, [C.c_void_p, C.POINTER(KernelSpec), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    # multivariate_normal of layers.py:342 summed over the outputs
    "dsdgp_gpr_bound": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    # layers.py:333-334
    "dsdgp_gpr_var": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_double, C.c_void_p]),
    # the sparse conditional with q_sqrt = None (layers.py:200, 249-260) and its reverse pass; the caller holds the scratch block
    "dsdgp_sparse_conditional_scratch_bytes": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "dsdgp_sparse_conditional": (C.c_int, [C.c_void_p, C.POINTER(KernelSpec), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_int)]),
    "dsdgp_sparse_conditional_grad": (C.c_int, [C.c_void_p, C.POINTER(KernelSpec), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                                C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    # DGP_Base over SGPMC layers (dgp.py:42-98, layers.py:249-260): the whole stack forward and backward in a block the caller holds
    "dsdgp_sizeof_stack_desc": (C.c_int, []),
    "dsdgp_stack_scratch_bytes": (C.c_int, [C.POINTER(StackDesc), C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "dsdgp_stack_propagate": (C.c_int, [C.c_void_p, C.POINTER(StackDesc), C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p),
                                        C.c_uint64, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "dsdgp_stack_logdensity": (C.c_int, [C.c_void_p, C.POINTER(StackDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                         C.POINTER(C.c_void_p), C.c_uint64, C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_int)]),
    "dsdgp_stack_hop": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "dsdgp_stack_hop_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double,
                                      C.c_void_p, C.c_void_p]),
    "dsdgp_sghmc_step": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double]),
    # pathwise (Matheron) function draws: the fused evaluation and the update weights (no reference counterpart)
    "dsdgp_pathwise_eval": (C.c_int, [C.c_void_p, C.POINTER(KernelSpec), C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                      C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]),
    "dsdgp_pathwise_scratch_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "dsdgp_pathwise_weights": (C.c_int, [C.c_void_p, C.POINTER(KernelSpec), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int)]),
    "dsdgp_model_set_grad_first_layer":(C.c_int, [C.c_void_p, C.c_int32]),
    "dsdgp_model_set_grad_q_only": (C.c_int, [C.c_void_p, C.c_int32]),
    "dsdgp_model_track_theta": (C.c_int, [C.c_void_p, C.c_int]),
    "dsdgp_model_theta_changed": (C.c_int, [C.c_void_p]),
    "dsdgp_allreduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
}

BUCKET_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p)

EXPORTED_SYMBOLS = tuple(_PROTOS.keys())


def lib_path():
    return _LIB_PATH


def load():
    """dlopen libdsdgp.so and attach prototypes.  Raises if the library was not built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise DsdgpError(f"{_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(_LIB_PATH)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc):
    if rc == 0:
        return
    msg = load().dsdgp_last_error().decode("utf-8", "replace")
    if rc == ERR_NOT_SPD:
        raise CholeskyError(msg)
    raise DsdgpError(f"libdsdgp error {rc}: {msg}")
