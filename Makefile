# Top-level build: everything is built IN-TREE (the .so files travel to the GPU box with
# gpurun; they are git-ignored).  `python -c "import __graft_entry__ as g; g.build()"` runs this.
#
#   spz_amd/lib/libspz_amd.so    HIP kernels (spz_kernels.hip, spz_ply_kernels.hip, spz_median.hip, spz_filter.hip, spz_transform.hip, spz_merge.hip, spz_sort.hip, spz_decimate.hip, spz_tile.hip, spz_clean.hip, spz_align.hip, spz_render.hip, spz_render_backward.hip, spz_render_view_backward.hip, spz_locate.hip, spz_mesh.hip, spz_prune.hip, spz_metrics.hip, spz_refine.hip, spz_densify.hip, spz_photo.hip, spz_depth_loss.hip, spz_seed.hip, spz_plane.hip) + C ABI (spz_abi.hip, spz_hostpath.hip, spz_exchange.hip)   (hipcc, gfx950)
#   spz_amd/lib/libspz_host.so   C++ drop-in layer spz::saveSpz/loadSpz + gzip (g++, zlib)
#   spz_amd/spz*.so              Python module `spz` (pybind11) over the C++ layer
#   spz_amd/bin/{ply_to_spz,spz_to_ply,spz_info}   the reference's three CLI tools over the C++ layer (+ spz_filter, spz_transform, spz_merge, spz_sort, spz_decimate, spz_clean, spz_render, spz_prune, spz_compare, spz_tile, spz_align, spz_refine, spz_fit, spz_seed, spz_locate, spz_mesh, spz_level)
#   oracle/liboracle.so, oracle/_ref/libspz_ref.so   CPU checkers (tests only)

ROOT    := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
HIPCC   ?= /opt/rocm/bin/hipcc
CXX     ?= g++
PYTHON  ?= python3
ARCH    ?= gfx950
LIBDIR  := $(ROOT)spz_amd/lib
CSRC    := $(ROOT)spz_amd/csrc
INC     := $(ROOT)include

# -ffp-contract=off: bit-exact quantisation needs every a*b+c rounded twice.
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math \
            -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function -I$(INC)
CXXFLAGS := -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -I$(INC)

PYEXT   := $(shell $(PYTHON) -c "import sysconfig; print(sysconfig.get_config_var('EXT_SUFFIX'))")
PYINC   := $(shell $(PYTHON) -c "import sysconfig, pybind11; print('-I' + sysconfig.get_paths()['include'] + ' -I' + pybind11.get_include())")

all: device host python cli oracle

device: $(LIBDIR)/libspz_amd.so
host:   $(LIBDIR)/libspz_host.so
python: $(ROOT)spz_amd/spz$(PYEXT)
cli:    $(ROOT)spz_amd/bin/spz_tool $(ROOT)spz_amd/bin/dropin_user_test $(ROOT)spz_amd/bin/host_bench $(ROOT)spz_amd/bin/render_chain_host

DEVICE_SRCS := $(CSRC)/spz_kernels.hip $(CSRC)/spz_abi.hip $(CSRC)/spz_hostpath.hip $(CSRC)/spz_ply_kernels.hip $(CSRC)/spz_median.hip $(CSRC)/spz_exchange.hip $(CSRC)/spz_lz77.hip $(CSRC)/spz_inflate_dev.hip $(CSRC)/spz_place.hip $(CSRC)/spz_filter.hip $(CSRC)/spz_transform.hip $(CSRC)/spz_merge.hip $(CSRC)/spz_sort.hip $(CSRC)/spz_decimate.hip $(CSRC)/spz_tile.hip $(CSRC)/spz_clean.hip $(CSRC)/spz_align.hip $(CSRC)/spz_render.hip $(CSRC)/spz_render_backward.hip $(CSRC)/spz_render_view_backward.hip $(CSRC)/spz_locate.hip $(CSRC)/spz_mesh.hip $(CSRC)/spz_prune.hip $(CSRC)/spz_metrics.hip $(CSRC)/spz_refine.hip $(CSRC)/spz_densify.hip $(CSRC)/spz_photo.hip $(CSRC)/spz_depth_loss.hip $(CSRC)/spz_seed.hip $(CSRC)/spz_plane.hip
$(LIBDIR)/libspz_amd.so: $(DEVICE_SRCS) $(CSRC)/spz_densify_internal.hpp $(CSRC)/spz_photo_internal.hpp $(CSRC)/spz_image_tile.hpp $(CSRC)/spz_common.hpp $(CSRC)/spz_kernel_params.hpp $(CSRC)/spz_quant.hpp $(CSRC)/spz_sort_internal.hpp $(CSRC)/spz_render_internal.hpp $(CSRC)/spz_view_pass.hpp $(CSRC)/spz_view_backward_core.hpp $(CSRC)/spz_preprocess_backward_core.hpp $(CSRC)/spz_morton_walk.hpp $(CSRC)/spz_block_ops.hpp $(CSRC)/spz_xf.hpp $(CSRC)/spz_lz77_core.hpp $(CSRC)/spz_huff_core.hpp $(CSRC)/spz_inflate_core.hpp $(INC)/spz_amd.h
	mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(DEVICE_SRCS) -ldl

$(LIBDIR)/libspz_host.so: $(CSRC)/spz_host.cpp $(CSRC)/spz_ply.cpp $(CSRC)/spz_deflate.cpp $(CSRC)/spz_lz77_model.cpp $(CSRC)/spz_lz77_core.hpp $(CSRC)/spz_huff_core.hpp $(CSRC)/spz_deflate.hpp $(CSRC)/spz_inflate.cpp $(CSRC)/spz_inflate.hpp $(CSRC)/spz_inflate_core.hpp $(CSRC)/spz_host_util.hpp $(INC)/spz_amd_host.hpp $(INC)/spz_amd.h $(LIBDIR)/libspz_amd.so
	$(CXX) $(CXXFLAGS) -shared -o $@ $(CSRC)/spz_host.cpp $(CSRC)/spz_ply.cpp $(CSRC)/spz_deflate.cpp $(CSRC)/spz_lz77_model.cpp $(CSRC)/spz_inflate.cpp -L$(LIBDIR) -lspz_amd -lz -ldl -lpthread \
	    -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,/opt/rocm/lib

$(ROOT)spz_amd/spz$(PYEXT): $(CSRC)/spz_py.cpp $(CSRC)/spz_py_args.hpp $(INC)/spz_amd_host.hpp $(LIBDIR)/libspz_host.so
	$(CXX) $(CXXFLAGS) $(PYINC) -fvisibility=hidden -shared -o $@ $(CSRC)/spz_py.cpp \
	    -L$(LIBDIR) -lspz_host -lspz_amd -Wl,-rpath,'$$ORIGIN/lib' -Wl,-rpath,/opt/rocm/lib

$(ROOT)spz_amd/bin/spz_tool: $(CSRC)/spz_cli.cpp $(INC)/spz_amd_host.hpp $(LIBDIR)/libspz_host.so
	mkdir -p $(ROOT)spz_amd/bin
	$(CXX) $(CXXFLAGS) -o $@ $(CSRC)/spz_cli.cpp -L$(LIBDIR) -lspz_host -lspz_amd \
	    -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib
	for t in ply_to_spz spz_to_ply spz_info spz_filter spz_transform spz_merge spz_sort spz_decimate spz_clean spz_render spz_prune spz_compare spz_tile spz_align spz_refine spz_fit spz_seed spz_locate spz_mesh spz_level; do ln -sf spz_tool $(ROOT)spz_amd/bin/$$t; done

# A user program written against the reference's C++ API, built against the compat headers
# (tests/cpp/dropin_user.cpp; its expected output comes from the same source built against the reference).
$(ROOT)spz_amd/bin/dropin_user_test: $(ROOT)tests/cpp/dropin_user.cpp $(INC)/compat/load-spz.h $(LIBDIR)/libspz_host.so
	mkdir -p $(ROOT)spz_amd/bin
	$(CXX) $(CXXFLAGS) -I$(INC)/compat -o $@ $(ROOT)tests/cpp/dropin_user.cpp -L$(LIBDIR) -lspz_host -lspz_amd \
	    -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib

# The C++ boundary (host vectors in and out) timed without a language binding in the way.
$(ROOT)spz_amd/bin/host_bench: $(ROOT)tools/host_bench.cpp $(INC)/spz_amd_host.hpp $(LIBDIR)/libspz_host.so
	mkdir -p $(ROOT)spz_amd/bin
	$(CXX) $(CXXFLAGS) -o $@ $(ROOT)tools/host_bench.cpp -L$(LIBDIR) -lspz_host -lspz_amd -lpthread \
	    -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib

# The render backward's two per-Gaussian chains (preprocess_backward_one, view_backward_one: host-and-device functions)
# built for the host, a stand-alone program that tests/test_render_frustum_host.py runs over its scenes (CPU only).
$(ROOT)spz_amd/bin/render_chain_host: $(ROOT)tests/cpp/render_chain_host.cpp $(CSRC)/spz_preprocess_backward_core.hpp $(CSRC)/spz_view_backward_core.hpp $(CSRC)/spz_render_internal.hpp $(CSRC)/spz_common.hpp $(INC)/spz_amd.h
	mkdir -p $(ROOT)spz_amd/bin
	$(HIPCC) --cuda-host-only -x hip -O2 -std=c++17 -ffp-contract=off -Wall -Wno-unused-function -I$(INC) -o $@ \
	    $(ROOT)tests/cpp/render_chain_host.cpp

oracle:
	$(MAKE) -C $(ROOT)oracle

# Kernel ISA + resource usage for inspection (not part of `all`).
asm: $(CSRC)/spz_kernels.hip
	mkdir -p $(ROOT)build
	$(HIPCC) $(HIPFLAGS) -S --cuda-device-only -Rpass-analysis=kernel-resource-usage \
	    -o $(ROOT)build/spz_kernels.s $(CSRC)/spz_kernels.hip

clean:
	rm -rf $(LIBDIR) $(ROOT)build $(ROOT)spz_amd/spz*.so $(ROOT)spz_amd/bin
	$(MAKE) -C $(ROOT)oracle clean

.PHONY: fuzz fuzz-foreign view-grad-check gzip-campaign all device host python cli oracle asm clean

# The byte-identity of the multi-threaded gzip writer against zlib 1.2.11 on ~9 300 randomized inputs (host
# only, about twenty minutes on 8 cores); the result line goes to profiles/.
gzip-campaign: host python
	$(PYTHON) $(ROOT)tools/gzip_campaign.py --inputs 9300 | tee $(ROOT)profiles/gzip_campaign.json

# Host-side robustness: the gzip readers and the .ply header parser under AddressSanitizer + UBSan
# (CPU only; the GPU pool has no sanitizer support).  Mutated inputs; must finish without a report.
fuzz: $(LIBDIR)/libspz_amd.so
	mkdir -p $(ROOT)build
	for t in gunzip_fuzz ply_fuzz deflate_fuzz inflate_fuzz; do \
	  $(CXX) -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=gnu++17 -I$(INC) -o $(ROOT)build/$$t \
	    $(ROOT)tools/fuzz/$$t.cpp $(CSRC)/spz_host.cpp $(CSRC)/spz_ply.cpp $(CSRC)/spz_deflate.cpp $(CSRC)/spz_lz77_model.cpp $(CSRC)/spz_inflate.cpp -L$(LIBDIR) -lspz_amd -lz -ldl -lpthread \
	    -Wl,-rpath,$(abspath $(LIBDIR)) && ASAN_OPTIONS=detect_leaks=0 $(ROOT)build/$$t || exit 1; \
	done

# The view backward's one-Gaussian chain (spz_view_backward_core.hpp) built for the host under ASan + UBSan, a stand-alone
# program, over the four scenes of the GPU test against tests/view_grad_ref.py (CPU only).
view-grad-check:
	mkdir -p $(ROOT)build
	$(HIPCC) --cuda-host-only -x hip -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	    -fno-omit-frame-pointer -I$(INC) -o $(ROOT)build/view_grad_check $(ROOT)tools/view_grad_check.cpp \
	    -fsanitize=address,undefined
	ASAN_OPTIONS=detect_leaks=0 $(PYTHON) $(ROOT)tools/view_grad_check.py $(ROOT)build/view_grad_check

# The decoder source both inflate readers share, under ASan + UBSan, over the crafted members of tests/deflate_craft.py
# (valid deflate no zlib writes, and members invalid in one chosen way), at the device reader's size and the host reader's.
fuzz-foreign:
	mkdir -p $(ROOT)build/foreign_small $(ROOT)build/foreign_large
	$(CXX) -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=gnu++17 -I$(INC) -o $(ROOT)build/inflate_foreign \
	    $(ROOT)tools/fuzz/inflate_foreign.cpp $(CSRC)/spz_inflate.cpp -lz -lpthread
	$(PYTHON) $(ROOT)tests/deflate_craft.py $(ROOT)build/foreign_small 1150000
	$(PYTHON) $(ROOT)tests/deflate_craft.py $(ROOT)build/foreign_large
	ASAN_OPTIONS=detect_leaks=0 $(ROOT)build/inflate_foreign $(ROOT)build/foreign_small/*.gz
	ASAN_OPTIONS=detect_leaks=0 $(ROOT)build/inflate_foreign $(ROOT)build/foreign_large/*.gz
