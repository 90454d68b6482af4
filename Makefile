# Build libslamhip.so (gfx950 only): one object per translation unit, compiler temporaries (ISA, resource reports) under build/.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
CSRC  := slam_decomposition_amd/csrc
UNITS := slam_hip slam_v2_host slam_smush_host slam_geometry slam_analytic slam_q3_host slam_ham_host slam_hams_host slam_comm
OBJS  := $(UNITS:%=build/%.o)
OUT   := slam_decomposition_amd/lib/libslamhip.so
# -amdgpu-mfma-vgpr-form: the metric update's MFMAs (h_update_mfma) accumulate in VGPRs, where the metric lives, also in the kernels
# that park spills in AGPRs (span 3); without it the compiler moves every block through AGPRs there (+50 registers, +212 instructions)
FLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -mllvm -amdgpu-mfma-vgpr-form

all: $(OUT)

# the compiler's remarks (and, on failure, its errors) go to the unit's report; header dependencies to build/<unit>.d
build/%.o: $(CSRC)/%.hip
	@mkdir -p build
	$(HIPCC) $(FLAGS) -c -save-temps=obj -Rpass-analysis=kernel-resource-usage -MMD -MF build/$*.d -o $@ $< 2> build/$*.resource_usage.txt || (cat build/$*.resource_usage.txt; exit 1)

$(OUT): $(OBJS)
	mkdir -p slam_decomposition_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -fPIC -shared -o build/libslamhip.so $(OBJS) -ldl
	cat $(UNITS:%=build/%.resource_usage.txt) > build/resource_usage.txt
	cp build/libslamhip.so $(OUT)

-include $(OBJS:.o=.d)

clean:
	rm -rf build $(OUT)

.PHONY: all clean

# host-side AddressSanitizer + UBSan build, driven through every C-ABI entry point's no-GPU paths (CPU only)
asan:
	bash tools/asan_host.sh

.PHONY: asan
