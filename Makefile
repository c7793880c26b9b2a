# Build of the MI355X bidirectional path tracer.
#   libbdpt.so  : HIP kernels (gfx950) + C-ABI + host utilities   (the product)
#   smallpt     : headless C host program, drop-in for smallpt_cpu.c's main/IdleFunc loop
#   oracle/liboracle.so : CPU restatement used by tests/bench only (never linked by the product)
#   oracle/_ref/libref.so : the reference's own kernels compiled in place as host C++, where the
#                           reference tree exists (tests only; see "The reference build" below)
# Everything builds with -ffp-contract=off: results must match the oracle bit for bit.

PKG      := gpu_bidirectional_raytracer_amd
CSRC     := $(PKG)/csrc
BUILD    ?= $(PKG)/_build
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
CC       ?= gcc
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize \
            -Wall -Wno-unused-function $(EXTRA_HIPFLAGS)
CFLAGS   := -O2 -std=gnu11 -fPIC -ffp-contract=off -Wall -Wextra -Wno-unused-parameter

LIB      ?= $(PKG)/libbdpt.so
HOST     := $(PKG)/smallpt
ORACLE   := oracle/liboracle.so

CHECKS   := tests/native/hw_exact_check tests/native/leaf_check tests/native/leaf_check_coarse \
            tests/native/plan_tiles_check

all: $(LIB) $(HOST) $(ORACLE) $(CHECKS)

# exhaustive hardware checks run by tests/test_gpu_hw_exact.py (test infrastructure)
tests/native/hw_exact_check: tests/native/hw_exact_check.hip $(CSRC)/bdpt_math.h
	$(HIPCC) --offload-arch=$(ARCH) -O3 -ffp-contract=off -o $@ $<

# the leaf device functions against plain statements, run by tests/test_gpu_leaf.py; the second
# binary checks bdpt_sincos_tab with the 256-entry table
LEAF_DEPS := tests/native/leaf_check.hip $(CSRC)/bdpt_leaf.h $(CSRC)/bdpt_math.h $(CSRC)/bdpt_sincos_table.h $(CSRC)/bdpt_device.h
tests/native/leaf_check: $(LEAF_DEPS)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -ffp-contract=off -pthread -o $@ $<

tests/native/leaf_check_coarse: $(LEAF_DEPS)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -ffp-contract=off -pthread -DBDPT_SC_COARSE=1 -o $@ $<

# the planner of masked path passes (host code only), run by tests/test_plan_tiles.py
tests/native/plan_tiles_check: tests/native/plan_tiles_check.cpp $(CSRC)/bdpt_plan.h $(CSRC)/bdpt_device.h include/bdpt.h
	$(HIPCC) -O1 -std=c++17 -o $@ $<

$(BUILD):
	mkdir -p $(BUILD)

# the arithmetic stated once for the HIP kernels and the CPU backend, and what each side brings
EYE_DEPS := $(CSRC)/bdpt_sides.h $(CSRC)/bdpt_eye.h $(CSRC)/bdpt_filter.h

$(BUILD)/bdpt_kernels.o: $(CSRC)/bdpt_kernels.hip $(CSRC)/bdpt_device.h $(CSRC)/bdpt_math.h $(CSRC)/bdpt_sincos_table.h $(CSRC)/bdpt_leaf.h $(CSRC)/bdpt_frame_kernels.h $(EYE_DEPS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the same file once more for launches over a tile list (BDPT_TILES: only the generic and the BVH
# instance of the path kernel with the tile-list code, bdpt_path_tiles_kernel_table)
$(BUILD)/bdpt_kernels_tiles.o: $(CSRC)/bdpt_kernels.hip $(CSRC)/bdpt_device.h $(CSRC)/bdpt_math.h $(CSRC)/bdpt_sincos_table.h $(CSRC)/bdpt_leaf.h $(EYE_DEPS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DBDPT_TILES=1 -c $< -o $@

# the path kernel's sources as strings, for scene-specialised kernels compiled at run time
$(CSRC)/bdpt_jit_src.h: tools/embed_jit_sources.py $(CSRC)/bdpt_kernels.hip $(CSRC)/bdpt_device.h $(CSRC)/bdpt_math.h $(CSRC)/bdpt_sincos_table.h $(CSRC)/bdpt_leaf.h
	python3 tools/embed_jit_sources.py $@

CTX_DEPS := $(CSRC)/bdpt_ctx.h $(CSRC)/bdpt_device.h $(CSRC)/bdpt_plan.h $(CSRC)/bdpt_jit_plan.h $(CSRC)/bdpt_cpu.h include/bdpt.h
$(BUILD)/bdpt_host.o: $(CSRC)/bdpt_host.cpp $(CTX_DEPS) $(CSRC)/bdpt_bvh.h $(EYE_DEPS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/bdpt_jit.o: $(CSRC)/bdpt_jit.cpp $(CTX_DEPS) $(CSRC)/bdpt_jit_src.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/bdpt_frame.o: $(CSRC)/bdpt_frame.cpp $(CTX_DEPS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/bdpt_bvh.o: $(CSRC)/bdpt_bvh.cpp $(CSRC)/bdpt_bvh.h include/bdpt.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/bdpt_cpu.o: $(CSRC)/bdpt_cpu.cpp $(CSRC)/bdpt_cpu.h $(EYE_DEPS) include/bdpt.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/bdpt_util.o: $(CSRC)/bdpt_util.c include/bdpt.h | $(BUILD)
	$(CC) $(CFLAGS) -c $< -o $@

$(BUILD)/bdpt_ckpt.o: $(CSRC)/bdpt_ckpt.c include/bdpt.h | $(BUILD)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIB): $(BUILD)/bdpt_kernels.o $(BUILD)/bdpt_host.o $(BUILD)/bdpt_jit.o $(BUILD)/bdpt_frame.o $(BUILD)/bdpt_bvh.o $(BUILD)/bdpt_cpu.o $(BUILD)/bdpt_util.o $(BUILD)/bdpt_ckpt.o $(BUILD)/bdpt_kernels_tiles.o
	mkdir -p $(dir $(LIB))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -lm -ldl

$(HOST): $(CSRC)/smallpt.c $(CSRC)/smallpt_app.h include/bdpt.h $(LIB)
	$(CC) $(CFLAGS) -o $@ $< -L$(PKG) -lbdpt -lm -Wl,-rpath,'$$ORIGIN'

# the optional display: X11 + GLX viewer over HIP-GL interop; built when the
# image has the GL/X11 headers (libbdpt itself never links OpenGL)
GLHOST   := $(PKG)/smallpt_gl
GL_OK    := $(shell test -f /usr/include/GL/glx.h -a -f /usr/include/X11/Xlib.h && echo 1)
ifeq ($(GL_OK),1)
all: $(GLHOST)
endif
$(GLHOST): $(CSRC)/smallpt_gl.c $(CSRC)/smallpt_app.h include/bdpt.h $(LIB)
	$(CC) $(CFLAGS) -o $@ $< -L$(PKG) -lbdpt -lGL -lX11 -lm -Wl,-rpath,'$$ORIGIN'

$(ORACLE): oracle/bdpt_oracle.c include/bdpt.h
	$(CC) -O2 -std=gnu11 -fPIC -shared -fopenmp -ffp-contract=off -Wall -o $@ $< -lm

# The reference build (test infrastructure; tests/test_ref_parity.py, tests/golden/make_ref_golden.py).
# The reference's src/device.cu and src/MersenneTwister_kernel.cu compile, unmodified and in place,
# as host C++ behind oracle/ref_shim.h; oracle/ref_driver.cpp replays the launches of
# smallpt_cpu.c.  The four -D renames repair identifiers the reference left stale when it renamed
# its locals (device.cu:260,279-300,670 use hitPoint/currentRay/inilight/pC; the declarations are
# hit_point/current_ray/ini_light/rand_count); every other use of those names is a consistent local
# or parameter, so the global rename is exact.  Nothing of the reference is copied: oracle/_ref/ is
# ignored by git, and where BDPT_REFERENCE does not exist the step is skipped and whatever
# oracle/_ref/ holds is left alone.
#   libref.so      : cos/sin/pow of a float evaluated as (float)f((double)x) (the project's contract)
#   libref_libm.so : the same calls resolved to the platform's float overloads (measured only)
#   libref_host.so : the reference's src/display_func.c (ReadScene, UpdateCamera, KeyFunc,
#                    SpecialFunc) as C, against the empty GL/CUDA stand-ins of oracle/ref_stubs/
#                    and the callbacks of oracle/ref_host_driver.c
BDPT_REFERENCE ?= /root/reference
REFDIR     := oracle/_ref
REF_SRCS   := $(BDPT_REFERENCE)/src/device.cu $(BDPT_REFERENCE)/src/MersenneTwister_kernel.cu
REF_RENAME := -DhitPoint=hit_point -DcurrentRay=current_ray -Dinilight=ini_light -DpC=rand_count
REF_FLAGS  := -O2 -ffp-contract=off -fPIC -shared -w -Wl,-Bsymbolic -include oracle/ref_shim.h \
              -I$(BDPT_REFERENCE)/include $(REF_RENAME)
ifneq ($(wildcard $(BDPT_REFERENCE)/src/device.cu),)
all: $(REFDIR)/libref.so $(REFDIR)/libref_libm.so $(REFDIR)/libref_host.so

$(REFDIR)/libref.so: $(REF_SRCS) oracle/ref_driver.cpp oracle/ref_shim.h
	mkdir -p $(REFDIR)
	g++ $(REF_FLAGS) -o $@ -x c++ $(REF_SRCS) oracle/ref_driver.cpp -lm

$(REFDIR)/libref_libm.so: $(REF_SRCS) oracle/ref_driver.cpp oracle/ref_shim.h
	mkdir -p $(REFDIR)
	g++ $(REF_FLAGS) -DREF_PLATFORM_LIBM -o $@ -x c++ $(REF_SRCS) oracle/ref_driver.cpp -lm

$(REFDIR)/libref_host.so: $(BDPT_REFERENCE)/src/display_func.c oracle/ref_host_driver.c $(wildcard oracle/ref_stubs/*.h oracle/ref_stubs/GL/*.h)
	mkdir -p $(REFDIR)
	gcc -O2 -std=gnu11 -ffp-contract=off -fPIC -shared -w -Wl,-Bsymbolic -Ioracle/ref_stubs \
	    -I$(BDPT_REFERENCE)/include -o $@ $(BDPT_REFERENCE)/src/display_func.c oracle/ref_host_driver.c -lm
endif

# Sanitizer build (GPU sanitizers are not available on the pool): the C host, the host
# utilities and the CPU backend under AddressSanitizer + UBSan through a HIP-free context layer,
# plus the oracle driven against the same CPU backend.  Run by tests/test_asan.py.
ASAN_FLAGS := -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -g -O1 -ffp-contract=off
ASAN_DIR   := tests/native/_asan
asan: $(ASAN_DIR)/smallpt_asan $(ASAN_DIR)/oracle_asan $(ASAN_DIR)/aov_asan $(ASAN_DIR)/denoise_asan $(ASAN_DIR)/reproject_asan \
      $(ASAN_DIR)/preview_asan $(ASAN_DIR)/noise_asan $(ASAN_DIR)/tiles_asan $(ASAN_DIR)/denoise_noise_asan \
      $(ASAN_DIR)/chain_asan $(ASAN_DIR)/follow_asan

$(ASAN_DIR):
	mkdir -p $(ASAN_DIR)

$(ASAN_DIR)/%.o: $(CSRC)/%.c include/bdpt.h | $(ASAN_DIR)
	$(CC) $(ASAN_FLAGS) -std=gnu11 -c $< -o $@

$(ASAN_DIR)/bdpt_cpu.o: $(CSRC)/bdpt_cpu.cpp $(CSRC)/bdpt_cpu.h $(EYE_DEPS) include/bdpt.h | $(ASAN_DIR)
	g++ $(ASAN_FLAGS) -std=c++17 -c $< -o $@

# the HIP-free context layer: every entry point smallpt calls, the frame services included, in
# tests/native/asan_cpu_abi.cpp.  It used to be a chain of files, each including the one before and
# adding a service's entry points, with asan_cpu_abi_noise.cpp on top; a tests/ tree that still has
# the chain (the sanitizer tests as they stood before the layer became one file) builds its top.
# asan_cpu_abi_denoise_noise.cpp includes asan_cpu_abi_noise.cpp and adds bdpt_denoise_noise (smallpt
# --denoise-noise); asan_cpu_abi_follow.cpp is the top now: it includes that one and adds
# bdpt_history_follow and bdpt_history_motion (smallpt --reproject-follow).
ASAN_ABI_SRC := $(firstword $(wildcard tests/native/asan_cpu_abi_follow.cpp) $(wildcard tests/native/asan_cpu_abi_denoise_noise.cpp) $(wildcard tests/native/asan_cpu_abi_noise.cpp) tests/native/asan_cpu_abi.cpp)
$(ASAN_DIR)/asan_cpu_abi.o: $(ASAN_ABI_SRC) $(wildcard tests/native/asan_cpu_abi*.cpp) $(CSRC)/bdpt_cpu.h include/bdpt.h | $(ASAN_DIR)
	g++ $(ASAN_FLAGS) -std=c++17 -c $< -o $@

$(ASAN_DIR)/bdpt_oracle.o: oracle/bdpt_oracle.c include/bdpt.h | $(ASAN_DIR)
	$(CC) $(ASAN_FLAGS) -std=gnu11 -c $< -o $@

$(ASAN_DIR)/smallpt_asan: $(ASAN_DIR)/smallpt.o $(ASAN_DIR)/bdpt_util.o $(ASAN_DIR)/bdpt_ckpt.o $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/asan_cpu_abi.o
	g++ $(ASAN_FLAGS) -o $@ $^ -lm -pthread

$(ASAN_DIR)/oracle_asan: tests/native/oracle_asan.c $(ASAN_DIR)/bdpt_oracle.o $(ASAN_DIR)/bdpt_util.o $(ASAN_DIR)/bdpt_ckpt.o $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/asan_cpu_abi.o
	g++ $(ASAN_FLAGS) -x c -std=gnu11 -c $< -o $(ASAN_DIR)/oracle_asan_main.o
	g++ $(ASAN_FLAGS) -o $@ $(ASAN_DIR)/oracle_asan_main.o $(filter %.o,$^) -lm -pthread

# the CPU backend's feature buffers (bdpt_cpu_render_aov) driven directly; tests/test_aov_asan.py
$(ASAN_DIR)/aov_asan: tests/native/aov_asan.cpp $(CSRC)/bdpt_cpu.h include/bdpt.h $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o
	g++ $(ASAN_FLAGS) -std=c++17 -o $@ $< $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o -lm -pthread

# the CPU backend's denoiser (bdpt_cpu_denoise) driven directly; tests/test_denoise_asan.py
$(ASAN_DIR)/denoise_asan: tests/native/denoise_asan.cpp $(CSRC)/bdpt_cpu.h include/bdpt.h $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o
	g++ $(ASAN_FLAGS) -std=c++17 -o $@ $< $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o -lm -pthread

# the CPU backend's history and reprojection driven directly; tests/test_reproject_asan.py
$(ASAN_DIR)/reproject_asan: tests/native/reproject_asan.cpp $(CSRC)/bdpt_cpu.h include/bdpt.h $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o
	g++ $(ASAN_FLAGS) -std=c++17 -o $@ $< $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o -lm -pthread

# the CPU backend's sphere-following history (bdpt_cpu_history_follow) driven directly; tests/test_follow_asan.py
$(ASAN_DIR)/follow_asan: tests/native/follow_asan.cpp $(CSRC)/bdpt_cpu.h include/bdpt.h $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o
	g++ $(ASAN_FLAGS) -std=c++17 -o $@ $< $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o -lm -pthread

# the CPU backend's denoised preview (bdpt_cpu_preview_denoise) driven directly; tests/test_preview_asan.py
$(ASAN_DIR)/preview_asan: tests/native/preview_asan.cpp $(CSRC)/bdpt_cpu.h include/bdpt.h $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o
	g++ $(ASAN_FLAGS) -std=c++17 -o $@ $< $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o -lm -pthread

# the CPU backend's noise estimate (bdpt_cpu_noise_*) driven directly; tests/test_noise_asan.py
$(ASAN_DIR)/noise_asan: tests/native/noise_asan.cpp $(CSRC)/bdpt_cpu.h include/bdpt.h $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o
	g++ $(ASAN_FLAGS) -std=c++17 -o $@ $< $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o -lm -pthread

# the CPU backend's noise-guided denoiser (bdpt_cpu_denoise_noise) driven directly; tests/test_denoise_noise_asan.py
$(ASAN_DIR)/denoise_noise_asan: tests/native/denoise_noise_asan.cpp $(CSRC)/bdpt_cpu.h include/bdpt.h $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o
	g++ $(ASAN_FLAGS) -std=c++17 -o $@ $< $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o -lm -pthread

# the CPU backend's chain buffers and the denoiser guided through them (bdpt_cpu_render_chain,
# bdpt_cpu_denoise with BDPT_DENOISE_THROUGH) driven directly; tests/test_chain_asan.py
$(ASAN_DIR)/chain_asan: tests/native/chain_asan.cpp $(CSRC)/bdpt_cpu.h include/bdpt.h $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o
	g++ $(ASAN_FLAGS) -std=c++17 -o $@ $< $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o -lm -pthread

# the CPU backend's masked path passes (bdpt_cpu_path_passes with a tile mask) driven directly; tests/test_tiles_asan.py
$(ASAN_DIR)/tiles_asan: tests/native/tiles_asan.cpp $(CSRC)/bdpt_cpu.h include/bdpt.h $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o
	g++ $(ASAN_FLAGS) -std=c++17 -o $@ $< $(ASAN_DIR)/bdpt_cpu.o $(ASAN_DIR)/bdpt_util.o -lm -pthread

clean:
	rm -rf $(BUILD) $(LIB) $(HOST) $(ORACLE) $(CHECKS) $(CSRC)/bdpt_jit_src.h $(ASAN_DIR)

# A/B variants for the GPU bench harness: make variant NAME=x EXTRA_HIPFLAGS="..."
variant:
	$(MAKE) BUILD=variants/$(NAME)/_build LIB=variants/$(NAME)/libbdpt.so variants/$(NAME)/libbdpt.so

.PHONY: all clean variant asan
