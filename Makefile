# Build libs2c.so (HIP kernels for gfx950 + host parser/planner/generator) in-tree.
# Used by __graft_entry__.build(); also `make -j8` by hand.
HIPCC   ?= /opt/rocm/bin/hipcc
CXX     ?= g++
ARCH    ?= gfx950
SRC      = sam2consensus_amd/csrc
OUT      = sam2consensus_amd/libs2c.so
BUILD    = build
CXXFLAGS = -O3 -std=c++17 -fPIC -pthread -Wall -Wextra -Iinclude
HIPFLAGS = -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -ffp-contract=off -Iinclude \
           -Wno-unused-result
LINK     = $(HIPCC) -shared -fPIC --offload-arch=$(ARCH) $^ -lz -lpthread -o $@

# the one list of host sources (every csrc/*.cpp) and of kernel sources
HOSTSRC  = $(wildcard $(SRC)/*.cpp)
HOSTOBJ  = $(HOSTSRC:$(SRC)/%.cpp=$(BUILD)/%.o)
KERNELS  = s2c_reads s2c_tile s2c_dense s2c_bodies s2c_table s2c_sites s2c_runs s2c_ins s2c_links s2c_dels
KOBJ     = $(KERNELS:%=$(BUILD)/%.o)

all: $(OUT)

$(BUILD)/%.o: $(SRC)/%.cpp $(SRC)/s2c_host_internal.h include/s2c.h | $(BUILD)
	$(CXX) $(CXXFLAGS) -c $< -o $@

# (every kernel's resource remarks checked: a spill fails the build, scripts/check_spills.py)
$(BUILD)/%.o: $(SRC)/%.hip $(SRC)/s2c_common.h $(SRC)/s2c_text.h include/s2c.h scripts/check_spills.py | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(BUILD)/$*.usage || { cat $(BUILD)/$*.usage; exit 1; }
	python3 scripts/check_spills.py $(BUILD)/$*.usage || { rm -f $@; exit 1; }

$(OUT): $(HOSTOBJ) $(KOBJ)
	$(LINK)

$(BUILD):
	mkdir -p $(BUILD)

# Diagnostic and experiment builds: libs2c_<suffix>.so = the host objects, the kernels named in
# DIAG_<suffix> rebuilt with DEFS_<suffix> (objects build/<kernel>_<suffix>.o), the others as built.
#   prof      phase clocks of k_tile_dense (S2C_LIB=libs2c_prof.so, scripts/prof_dense.py)
#   poison    every kernel fills its workgroup's LDS with 0xA5 at entry (S2C_LIB=libs2c_poison.so;
#             the GPU suite once under it shows no kernel reads LDS it did not write in that launch)
#   variant   k_reads, k_tile_dense and k_tile with extra defines (V=name VDEFS='-D...'): libs2c_$(V).so
V     ?= var
VDEFS ?=
DIAG_prof   = s2c_dense s2c_tile
DEFS_prof   = $(VDEFS) -DS2C_PROF
DIAG_poison = $(KERNELS)
DEFS_poison = -DS2C_LDS_POISON
DIAG_$(V)   = s2c_reads s2c_dense s2c_tile
DEFS_$(V)   = $(VDEFS)
prof: sam2consensus_amd/libs2c_prof.so
poison: sam2consensus_amd/libs2c_poison.so
variant: sam2consensus_amd/libs2c_$(V).so

define DIAG_RULES
$$(BUILD)/%_$(1).o: $$(SRC)/%.hip $$(SRC)/s2c_common.h $$(SRC)/s2c_text.h include/s2c.h FORCE | $$(BUILD)
	$$(HIPCC) $$(HIPFLAGS) $$(DEFS_$(1)) -c $$< -o $$@
sam2consensus_amd/libs2c_$(1).so: $$(HOSTOBJ) $$(filter-out $$(DIAG_$(1):%=$$(BUILD)/%.o),$$(KOBJ)) $$(DIAG_$(1):%=$$(BUILD)/%_$(1).o)
	$$(LINK)
endef
$(foreach s,$(sort prof poison $(V)),$(eval $(call DIAG_RULES,$(s))))

# kernel resource usage (VGPR/SGPR/LDS/occupancy) and ISA for inspection
ISA_DIR ?= /tmp/s2c_isa
isa:
	mkdir -p $(ISA_DIR)
	for f in $(KERNELS); do \
	  $(HIPCC) $(HIPFLAGS) -c $(SRC)/$$f.hip -o $(ISA_DIR)/$$f.o -save-temps=obj \
	    -Rpass-analysis=kernel-resource-usage 2> $(ISA_DIR)/$$f.resource_usage.txt; done

clean:
	rm -rf $(BUILD) $(OUT)

FORCE:   # (a diagnostic object is rebuilt every time: its defines come from the command line)
.PHONY: all clean isa prof variant poison FORCE
