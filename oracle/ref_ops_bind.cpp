// TEST INFRASTRUCTURE -- Python surface of the REFERENCE's op classes, compiled for the CPU (oracle/ref_ops.py).
// Class names, constructor arguments and methods are the ones oracle/pconv_cpu.py restates, so a test can drive
// both with the same calls.  Two things differ from a plain binding, both on purpose:
//   * every object is constructed in zero-filled storage.  Some op classes read members before anything has set
//     them (sphere_slice_opt::reshape compares height_ on the first call); in zeroed storage such a read sees 0
//     whatever the allocator handed out before, so results do not depend on allocation history.
//   * the three context classes are held directly, not through the reference's *_shell wrappers (which allocate
//     the context with a plain new), and also expose the tables they hand to the ops (produce_param,
//     produce_param_group) so that a test can read them.
#include <torch/extension.h>

#include <cstdlib>
#include <memory>
#include <new>
#include <sstream>
#include <string>
#include <vector>

#include "main.hpp"

namespace py = pybind11;

// oracle/ref_shim/coop_selfcheck.cu
std::vector<float> coop_neighbour(int n, int blocks, int launches);
std::vector<float> coop_tree(std::vector<float> in);
std::vector<float> coop_shuffle(std::vector<float> in, int n);

namespace {

template <class T> struct ZeroedDelete {
  void operator()(T *p) const {
    p->~T();
    std::free(p);
  }
};
template <class T> using Zeroed = std::unique_ptr<T, ZeroedDelete<T>>;

template <class T, class... A> Zeroed<T> make_zeroed(A... a) {
  void *mem = std::calloc(1, sizeof(T));
  if (!mem) throw std::bad_alloc();
  try {
    return Zeroed<T>(new (mem) T(a...));
  } catch (...) {
    std::free(mem);
    throw;
  }
}

template <class T, class... A> py::class_<T, Zeroed<T>> op(py::module &m, const char *name) {
  return py::class_<T, Zeroed<T>>(m, name).def(py::init(&make_zeroed<T, A...>)).def("to", &T::to);
}

// what the ops' FromString* helpers parse back into a pointer
template <class C> std::string address_of(const C *c) {
  std::stringstream ss;
  ss << static_cast<const void *>(c);
  return ss.str();
}

template <class C> struct Context {
  Zeroed<C> ctx;
  std::string addr;
  explicit Context(Zeroed<C> c) : ctx(std::move(c)), addr(address_of(ctx.get())) {}
  void to(int device) { ctx->to(device); }
  void start_context(int width) { ctx->start_context(width); }
  std::string get_pointer() { return addr; }
  at::Tensor produce_fill_param(int height, int width) { return ctx->produce_param_fill(height, width); }
  std::vector<at::Tensor> produce_param(int channel, int height, int width, int pad) {
    return ctx->produce_param(channel, height, width, pad);
  }
};

template <class C> py::class_<Context<C>> context(py::module &m, const char *name) {
  return py::class_<Context<C>>(m, name)
      .def("to", &Context<C>::to)
      .def("start_context", &Context<C>::start_context)
      .def("addr", &Context<C>::get_pointer)
      .def("produce_fill_param", &Context<C>::produce_fill_param)
      .def("produce_param", &Context<C>::produce_param);
}

typedef std::vector<float> floats;

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "the reference's extension ops, one CPU thread per kernel grid (the masked convolution: cooperating fibers)";

  context<pseudo_context_opt>(m, "PseudoContextOp")
      .def(py::init([](int npart, int rt, floats weight, int device, bool timeit) {
        return new Context<pseudo_context_opt>(make_zeroed<pseudo_context_opt>(npart, rt, weight, device, timeit));
      }));
  context<pseudo_entropy_context_opt>(m, "PseudoEntropyContextOp")
      .def(py::init([](int npart, int rt, int context_version, floats weight, int device, bool timeit) {
        return new Context<pseudo_entropy_context_opt>(
            make_zeroed<pseudo_entropy_context_opt>(npart, rt, context_version, weight, device, timeit));
      }));
  context<entropy_context>(m, "EntropyContextOp")
      .def(py::init([](int npart, int rt, floats weight, int device, bool timeit) {
        return new Context<entropy_context>(make_zeroed<entropy_context>(npart, rt, weight, device, timeit));
      }))
      .def("produce_param_group",
           [](Context<entropy_context> &c, int height, int width) { return c.ctx->produce_param_group(height, width); });

  op<projects_opt, int, int, floats, floats, float, bool, int, bool>(m, "ProjectsOp")
      .def("forward", &projects_opt::forward_cuda)
      .def("backward", &projects_opt::backward_cuda);
  op<dtow_opt, int, bool, int, bool>(m, "DtowOp")
      .def("forward", &dtow_opt::forward_cuda)
      .def("backward", &dtow_opt::backward_cuda);
  op<context_reshape_opt, int, int, bool>(m, "ContextReshapeOp")
      .def("forward", &context_reshape_opt::forward_cuda)
      .def("backward", &context_reshape_opt::backward_cuda);
  op<entropy_gmm_opt, int, int, int, bool>(m, "EntropyGmmOp")
      .def("forward", &entropy_gmm_opt::forward_cuda)
      .def("backward", &entropy_gmm_opt::backward_cuda);
  op<mask_constrain_opt, int, int, int, bool>(m, "MaskConstrainOp")
      .def("forward", &mask_constrain_opt::forward_cuda)
      .def("backward", &mask_constrain_opt::backward_cuda);
  op<sphere_slice_opt, int, int, int, floats, int, bool>(m, "SphereSliceOp")
      .def("forward", &sphere_slice_opt::forward_cuda)
      .def("backward", &sphere_slice_opt::backward_cuda);
  op<sphere_uslice_opt, int, int, int, floats, int, bool>(m, "SphereUsliceOp")
      .def("forward", &sphere_uslice_opt::forward_cuda)
      .def("backward", &sphere_uslice_opt::backward_cuda);
  op<entropy_gmm_table_opt, int, float, int, float, float, int, bool>(m, "EntropyGmmTableOp")
      .def("forward", &entropy_gmm_table_opt::forward_cuda)
      .def("forward_batch", &entropy_gmm_table_opt::forward_batch_cuda);
  op<entropy_ctx_pad_run2_opt, int, int, int, bool, std::string, int, bool>(m, "EntropyCtxPadRun2Op")
      .def("restart", &entropy_ctx_pad_run2_opt::restart)
      .def("forward", &entropy_ctx_pad_run2_opt::forward_cuda);
  op<d_extract_opt2, int, int, bool, std::string, int, bool>(m, "DExtract2Op")
      .def("restart", &d_extract_opt2::restart)
      .def("forward", &d_extract_opt2::forward_cuda)
      .def("forward_batch", &d_extract_opt2::forward_batch_cuda);
  op<d_input_opt2, int, int, int, float, int, std::string, int, bool>(m, "DInput2Op")
      .def("restart", &d_input_opt2::restart)
      .def("forward", &d_input_opt2::forward_cuda);
  op<entropy_add_opt, int, int, int, int, std::string, int, bool>(m, "EntropyAddOp")
      .def("restart", &entropy_add_opt::restart)
      .def("forward", &entropy_add_opt::forward_cuda);
  // the masked convolution: blocks of 128 cooperating threads, run by oracle/ref_shim/coop_launch.cpp
  op<entropy_conv_opt2, int, int, int, int, int, int, int, int, std::string, int, bool>(m, "EntropyConv2Op")
      .def("restart", &entropy_conv_opt2::restart)
      .def("forward", &entropy_conv_opt2::forward_cuda)
      .def("forward_act", &entropy_conv_opt2::forward_act_cuda)
      .def("forward_batch", &entropy_conv_opt2::forward_cuda_batch)
      .def("forward_act_batch", &entropy_conv_opt2::forward_act_cuda_batch);
  // the launcher's self-check (oracle/ref_shim/coop_selfcheck.cu)
  m.def("coop_neighbour", &coop_neighbour);
  m.def("coop_tree", &coop_tree);
  m.def("coop_shuffle", &coop_shuffle);
  op<pseudo_pad_opt, int, int, std::string, int, bool>(m, "PseudoPadOp")
      .def("forward", &pseudo_pad_opt::forward_cuda)
      .def("backward", &pseudo_pad_opt::backward_cuda);
  op<pseudo_fill_opt, int, int, int, int, std::string, int, int, bool>(m, "PseudoFillOp")
      .def("forward", &pseudo_fill_opt::forward_cuda)
      .def("backward", &pseudo_fill_opt::backward_cuda);
  op<pseudo_entropy_pad_opt, int, int, std::string, int, bool>(m, "PseudoEntropyPadOp")
      .def("forward", &pseudo_entropy_pad_opt::forward_cuda)
      .def("backward", &pseudo_entropy_pad_opt::backward_cuda);
  op<pseudo_quant_opt, int, int, int, float, int, int, float, std::string, int, bool>(m, "PseudoQuantOp")
      .def("forward", &pseudo_quant_opt::quant_forward_cuda)
      .def("backward", &pseudo_quant_opt::quant_backward_cuda);
  op<pseudo_dquant_opt, int, int, int, std::string, int, bool>(m, "PseudoDQuantOp")
      .def("forward", &pseudo_dquant_opt::forward_cuda);
}
