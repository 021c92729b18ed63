# Builds libleastereo_hip.so for gfx950 (MI355X) in-tree, plus the oracle's
# nothing-to-build marker.  `make -j8` here; the GPU box uses the prebuilt .so.
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall -Wno-unused-function \
            -Iinclude -Ileastereo_amd/csrc -munsafe-fp-atomics
SRC      := $(wildcard leastereo_amd/csrc/*.hip)
OBJ      := $(patsubst leastereo_amd/csrc/%.hip,build/obj/%.o,$(SRC))
LIB      := leastereo_amd/libleastereo_hip.so

all: $(LIB)

# the Winograd engines: SLP-packed f32 VALU (v_pk_*) beside MFMAs costs more issue
# cycles than the scalar pairs it replaces (MI355X_MICROARCH.md, filler prices)
build/obj/conv3d_wino.o build/obj/conv3d_wino2.o build/obj/conv3d_wino44.o: HIPFLAGS += -fno-slp-vectorize

build/obj/%.o: leastereo_amd/csrc/%.hip $(wildcard leastereo_amd/csrc/*.h) include/leastereo_hip.h include/leastereo_hip_tuning.h
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJ)

resource-usage: $(SRC)
	@mkdir -p build/ru
	for f in $(SRC); do $(HIPCC) $(HIPFLAGS) -c $$f -o build/ru/$$(basename $$f).o -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs:|AGPRs|ScratchSize|Occupancy|LDS Size" ; done

# Host-side AddressSanitizer build of the C-ABI boundary: every unit with
# ASan on its host side only (the device code is built as usual and never launched:
# the driver, tests/asan/capi_asan.cpp, drives each entry point through its argument
# checks and the host queries).  Runs on a machine without a GPU.
ASANFLAGS := -O1 -g -std=c++17 -fPIC --offload-arch=$(ARCH) -Iinclude -Ileastereo_amd/csrc -Xarch_host -fsanitize=address \
             -Xarch_host -fno-omit-frame-pointer
ASANOBJ   := $(patsubst leastereo_amd/csrc/%.hip,build/asan/%.o,$(SRC))

build/asan/%.o: leastereo_amd/csrc/%.hip $(wildcard leastereo_amd/csrc/*.h) include/leastereo_hip.h include/leastereo_hip_tuning.h
	@mkdir -p build/asan
	$(HIPCC) $(ASANFLAGS) -c $< -o $@

# one stand-alone driver per group of entry points (tests/asan/NAME.cpp -> build/asan/NAME), each
# linked with every unit: capi the ABI at large, disp_stats lea_disparity_regression_stats, lr the
# left-right check, loss the median and edge loss, transform the training transform, photo
# photometric consistency, scene whole-scene inference, refine the refinement, speckle the filter,
# pointcloud the point cloud, rectify the rectification, warp the view synthesis, dsm the surface model
ASANDRIVERS := capi_asan disp_stats_asan lr_asan loss_asan transform_asan photo_asan scene_asan refine_asan \
               speckle_asan pointcloud_asan rectify_asan warp_asan dsm_asan

$(ASANDRIVERS:%=build/asan/%_main.o): build/asan/%_main.o: tests/asan/%.cpp include/leastereo_hip.h include/leastereo_hip_tuning.h
	@mkdir -p build/asan
	$(HIPCC) $(ASANFLAGS) -c $< -o $@

$(ASANDRIVERS:%=build/asan/%): build/asan/%: build/asan/%_main.o $(ASANOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -fno-gpu-sanitize -fsanitize=address -o $@ $^

# one recipe line per driver, in the list's order
define ASANRUN
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/$(1)

endef

asan: $(addprefix build/asan/,$(ASANDRIVERS))
	$(foreach d,$(ASANDRIVERS),$(call ASANRUN,$(d)))

clean:
	rm -rf build $(LIB)

.PHONY: all clean resource-usage asan
