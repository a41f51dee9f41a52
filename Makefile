# Builds everything in-tree (no install step):
#   tsdf_amd/lib/libtsdf_hip.so   HIP kernels + C ABI (include/tsdf_amd.h), gfx950 only
#   tsdf_amd/lib/libtsdf_host.so  C++ class surface (TSDFVolume, GPURaycaster, Camera, ...) over the C ABI
#   oracle/libtsdf_oracle.so      CPU oracle (test infrastructure), oracle/_ref/*.so: what of the reference compiles from its own sources here (BilateralFilter.cpp, cuda_coordinate_transforms.cu), when the reference is mounted
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
# -ffp-contract=off: every fp32 op rounds on its own, in the reference's order (parity contract)
HIPFLAGS  = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Iinclude -Itsdf_amd/csrc -Wall -Wno-unused-function
CSRC      = tsdf_amd/csrc
# `make DIAG=1`: a library with the host-side diagnostics of diagnostics.hip (TSDF_DEBUG_SORT / TSDF_DEBUG_BRICKS); not the product build
ifeq ($(DIAG),1)
HIPFLAGS += -DTSDF_DIAGNOSTICS
endif
HIP_SRCS  = $(CSRC)/diagnostics.hip $(CSRC)/volume.hip $(CSRC)/integrate.hip $(CSRC)/integrate_weighted.hip $(CSRC)/integrate_packed.hip $(CSRC)/weights.hip $(CSRC)/raycast.hip $(CSRC)/bilateral.hip $(CSRC)/icp.hip $(CSRC)/mcubes.hip $(CSRC)/pipeline.hip $(CSRC)/colour.hip $(CSRC)/classes.hip $(CSRC)/field.hip $(CSRC)/fuse.hip $(CSRC)/align.hip $(CSRC)/integrate_rays.hip $(CSRC)/mesh.hip $(CSRC)/mesh_scan.hip $(CSRC)/mesh_components.hip $(CSRC)/mesh_simplify.hip $(CSRC)/mesh_smooth.hip $(CSRC)/mesh_render.hip $(CSRC)/esdf.hip $(CSRC)/explore.hip $(CSRC)/reach.hip $(CSRC)/objects.hip $(CSRC)/scene_flow.hip $(CSRC)/snapshot.hip $(CSRC)/columns.hip $(CSRC)/frame_diff.hip
HIP_OBJS  = $(HIP_SRCS:.hip=.o)
LIBDIR    = tsdf_amd/lib

# Host C++ (class surface).  A real Eigen wins when one is installed; otherwise the bundled
# minimal Eigen-compatible header is used.
CXX      ?= g++
HOSTDIR   = tsdf_amd/host
EIGEN_INC := $(shell for d in /usr/include/eigen3 /usr/local/include/eigen3; do [ -f $$d/Eigen/Core ] && echo -I$$d && break; done)
ifeq ($(EIGEN_INC),)
EIGEN_INC = -I$(HOSTDIR)/eigen_compat
endif
# the same for Sophus (used only by the ICPOdometry interface)
SOPHUS_INC := $(shell for d in /usr/include /usr/local/include; do [ -f $$d/sophus/se3.hpp ] && echo -I$$d && break; done)
ifeq ($(SOPHUS_INC),)
SOPHUS_INC = -I$(HOSTDIR)/sophus_compat
endif
HOSTFLAGS = -std=c++11 -O2 -pthread -ffp-contract=off -fPIC -Wall -Iinclude -I$(HOSTDIR)/include -I$(HOSTDIR)/third_party $(EIGEN_INC) $(SOPHUS_INC)
HOST_SRCS = $(wildcard $(HOSTDIR)/src/*.cpp)
HOST_OBJS = $(HOST_SRCS:.cpp=.o)

all: hip host oracle cpptest

host: $(LIBDIR)/libtsdf_host.so

$(HOSTDIR)/src/%.o: $(HOSTDIR)/src/%.cpp $(wildcard $(HOSTDIR)/include/*.hpp) $(wildcard $(HOSTDIR)/src/*.hpp) $(wildcard $(HOSTDIR)/eigen_compat/Eigen/*) $(wildcard $(HOSTDIR)/sophus_compat/sophus/*) $(wildcard $(HOSTDIR)/third_party/ICP_CUDA/*) include/tsdf_amd.h
	$(CXX) $(HOSTFLAGS) -c $< -o $@

$(LIBDIR)/libtsdf_host.so: $(HOST_OBJS) $(LIBDIR)/libtsdf_hip.so
	$(CXX) -shared -fPIC -pthread -o $@ $(HOST_OBJS) -L$(LIBDIR) -ltsdf_hip -lz -Wl,-rpath,'$$ORIGIN'

hip: $(LIBDIR)/libtsdf_hip.so

# integrate_packed_kernel is bound by its vector instruction stream: the scheduler's max-ILP strategy is worth 1-1.5 % there
# (0.0804 against 0.0816 ms; it costs the latency-bound ray kernels 13 % and the bilateral filter 11 %: those keep the default)
$(CSRC)/integrate_packed.o: HIPFLAGS += -mllvm -amdgpu-sched-strategy=max-ilp

$(CSRC)/%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.hpp) include/tsdf_amd.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/libtsdf_hip.so: $(HIP_OBJS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(HIP_OBJS) -ldl

oracle:
	$(MAKE) -C oracle -s all

CPPTESTS  = surface colour classes weight_cap field rays fuse align align_colour integrate_rays rays_colour mesh esdf explore reach objects components simplify smooth scene_flow snapshot weighted rolling columns render frame_diff
cpptest: $(CPPTESTS:%=build/test_%) build/kinfu_stream

# C++ driver of BASELINE configs[2] (TUM directory -> tsdf_pipeline_step, no Python): tools/kinfu_stream.cpp
build/kinfu_stream: tools/kinfu_stream.cpp $(LIBDIR)/libtsdf_host.so include/tsdf_amd.h
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -o $@ tools/kinfu_stream.cpp -L$(LIBDIR) -ltsdf_host -ltsdf_hip -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)'

# C++ checks through the class surface, one program per tests/cpp/test_NAME.cpp (run by tests/test_cpp_*.py and
# tests/test_colour_fusion.py on the GPU box)
build/test_%: tests/cpp/test_%.cpp $(LIBDIR)/libtsdf_host.so
	@mkdir -p build
	$(CXX) $(HOSTFLAGS) -o $@ $< -L$(LIBDIR) -ltsdf_host -ltsdf_hip -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)'

# Host-side sanitizer run of the scene-flow argument checks and refusals (they all return before any device work): a stand-alone
# program linked with scene_flow.hip alone, address and undefined-behaviour sanitizers on the host code only.  Needs no GPU.
sanitize-scene-flow: tests/cpp/scene_flow_refusals.cpp $(CSRC)/scene_flow.hip $(wildcard $(CSRC)/*.hpp) include/tsdf_amd.h
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Iinclude -I$(CSRC) -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -x hip $(CSRC)/scene_flow.hip tests/cpp/scene_flow_refusals.cpp -o build/scene_flow_refusals
	build/scene_flow_refusals

# The same for device_buffer.hpp (the grow-only array, release, free-all and the frame of a host variant): where there is no device every
# allocation fails, the one branch the GPU suite never takes; and for handle_order.hpp (a handle's event: create without a device, destroy
# of what was never created, join and wait with nothing pending) and handle_counters.hpp (a handle's counter block: create without a
# device, release of what was never or half created).  Headers only: nothing of the library is linked.
sanitize-device-buffer: tests/cpp/device_buffer_host.cpp $(CSRC)/device_buffer.hpp $(CSRC)/handle_order.hpp $(CSRC)/handle_counters.hpp include/tsdf_amd.h
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -Iinclude -I$(CSRC) -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -x hip tests/cpp/device_buffer_host.cpp -o build/device_buffer_host
	build/device_buffer_host

# The same for the headers of pure integer arithmetic, each with its stand-alone program tests/cpp/NAME_host.cpp:
#   sanitize-rolling     brick_shift.hpp: the rolling volume's brick arithmetic, shifts at the ends of the int32 range, formed in 64 bits.
#                        (The argument checks of tsdf_snapshot_select / tsdf_volume_shift live in snapshot.hip, which does not link
#                        without the rest of the library.)
#   sanitize-columns     columns_index.hpp: the column maps' cell and band arithmetic (map axes, strides, the reversed index, U * V * L in
#                        64 bits) against brute force on small grids and at the longest axis a map takes.
#   sanitize-render      raster_index.hpp: the mesh renderer's integer arithmetic (the snap, the twice-area, the edge functions, the
#                        top-left rule and the box clamp) at the ends of the coordinate range, on boxes wholly outside the image and
#                        against brute force over small images.
#   sanitize-frame-diff  frame_diff_index.hpp: the frame differences' integer arithmetic (the tolerance and its saturation, the states, the
#                        image neighbours, the clipped dilation window, the any-bit range test, W * H in 64 bits) at the ends of the
#                        ranges and against brute force.
# $(1): the target's suffix, $(2): the program's stem, $(3): the header
define SANITIZE_HEADER
sanitize-$(1): tests/cpp/$(2)_host.cpp $$(CSRC)/$(3)
	@mkdir -p build
	$$(HIPCC) --offload-arch=$$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -I$$(CSRC) -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -x hip tests/cpp/$(2)_host.cpp -o build/$(2)_host
	build/$(2)_host
endef
$(eval $(call SANITIZE_HEADER,rolling,rolling,brick_shift.hpp))
$(eval $(call SANITIZE_HEADER,columns,columns,columns_index.hpp))
$(eval $(call SANITIZE_HEADER,render,render,raster_index.hpp))
$(eval $(call SANITIZE_HEADER,frame-diff,frame_diff,frame_diff_index.hpp))

clean:
	rm -f $(HIP_OBJS) $(HOST_OBJS) $(LIBDIR)/*.so
	$(MAKE) -C oracle clean

.PHONY: all hip host oracle cpptest clean sanitize-scene-flow sanitize-device-buffer sanitize-rolling sanitize-columns sanitize-render sanitize-frame-diff
