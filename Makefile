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

build/asan/capi_asan_main.o: tests/asan/capi_asan.cpp include/leastereo_hip.h include/leastereo_hip_tuning.h
	@mkdir -p build/asan
	$(HIPCC) $(ASANFLAGS) -c $< -o $@

build/asan/capi_asan: build/asan/capi_asan_main.o $(ASANOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -fno-gpu-sanitize -fsanitize=address -o $@ $^

# the confidence head's entry (lea_disparity_regression_stats) has a driver of its own
build/asan/disp_stats_asan_main.o: tests/asan/disp_stats_asan.cpp include/leastereo_hip.h
	@mkdir -p build/asan
	$(HIPCC) $(ASANFLAGS) -c $< -o $@

build/asan/disp_stats_asan: build/asan/disp_stats_asan_main.o $(ASANOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -fno-gpu-sanitize -fsanitize=address -o $@ $^

# the left-right check's two entries (lea_disparity_regression_right, lea_disparity_lr_check)
build/asan/lr_asan_main.o: tests/asan/lr_asan.cpp include/leastereo_hip.h
	@mkdir -p build/asan
	$(HIPCC) $(ASANFLAGS) -c $< -o $@

build/asan/lr_asan: build/asan/lr_asan_main.o $(ASANOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -fno-gpu-sanitize -fsanitize=address -o $@ $^

# the edge-aware loss's three entries (lea_median5x5_f32, lea_edge_loss_f32, lea_edge_loss_grad_f32)
build/asan/loss_asan_main.o: tests/asan/loss_asan.cpp include/leastereo_hip.h
	@mkdir -p build/asan
	$(HIPCC) $(ASANFLAGS) -c $< -o $@

build/asan/loss_asan: build/asan/loss_asan_main.o $(ASANOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -fno-gpu-sanitize -fsanitize=address -o $@ $^

# the training transform's two entries (lea_train_transform_workspace_bytes, lea_train_transform_u8)
build/asan/transform_asan_main.o: tests/asan/transform_asan.cpp include/leastereo_hip.h
	@mkdir -p build/asan
	$(HIPCC) $(ASANFLAGS) -c $< -o $@

build/asan/transform_asan: build/asan/transform_asan_main.o $(ASANOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -fno-gpu-sanitize -fsanitize=address -o $@ $^

# photometric consistency's three entries (lea_photometric_workspace_bytes, lea_photometric_f32,
# lea_photometric_grad_f32)
build/asan/photo_asan_main.o: tests/asan/photo_asan.cpp include/leastereo_hip.h
	@mkdir -p build/asan
	$(HIPCC) $(ASANFLAGS) -c $< -o $@

build/asan/photo_asan: build/asan/photo_asan_main.o $(ASANOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -fno-gpu-sanitize -fsanitize=address -o $@ $^

# whole-scene inference's three entries (lea_standardize_tiles_workspace_bytes, lea_standardize_tiles_u8,
# lea_tile_blend_f32)
build/asan/scene_asan_main.o: tests/asan/scene_asan.cpp include/leastereo_hip.h
	@mkdir -p build/asan
	$(HIPCC) $(ASANFLAGS) -c $< -o $@

build/asan/scene_asan: build/asan/scene_asan_main.o $(ASANOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -fno-gpu-sanitize -fsanitize=address -o $@ $^

# the disparity refinement's two entries (lea_disparity_refine_workspace_bytes, lea_disparity_refine_f32)
build/asan/refine_asan_main.o: tests/asan/refine_asan.cpp include/leastereo_hip.h
	@mkdir -p build/asan
	$(HIPCC) $(ASANFLAGS) -c $< -o $@

build/asan/refine_asan: build/asan/refine_asan_main.o $(ASANOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -fno-gpu-sanitize -fsanitize=address -o $@ $^

# the speckle filter's two entries (lea_disparity_speckle_workspace_bytes, lea_disparity_speckle_f32)
build/asan/speckle_asan_main.o: tests/asan/speckle_asan.cpp include/leastereo_hip.h
	@mkdir -p build/asan
	$(HIPCC) $(ASANFLAGS) -c $< -o $@

build/asan/speckle_asan: build/asan/speckle_asan_main.o $(ASANOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -fno-gpu-sanitize -fsanitize=address -o $@ $^

asan: build/asan/capi_asan build/asan/disp_stats_asan build/asan/lr_asan build/asan/loss_asan build/asan/transform_asan build/asan/photo_asan \
      build/asan/scene_asan build/asan/refine_asan build/asan/speckle_asan
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/capi_asan
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/disp_stats_asan
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/lr_asan
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/loss_asan
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/transform_asan
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/photo_asan
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/scene_asan
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/refine_asan
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/asan/speckle_asan

clean:
	rm -rf build $(LIB)

.PHONY: all clean resource-usage asan
