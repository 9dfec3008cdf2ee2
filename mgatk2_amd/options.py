"""The options of the analyses of the heteroplasmy matrix as given, and which of them needs which. Nothing
heavy is imported (the command line reads this first); a range has its checker next to its analysis."""

from __future__ import annotations

from dataclasses import dataclass

FLAGS = {"call_variants": "--variants", "cluster": "--cluster", "clones": "--clones", "neighbors": "--neighbors",
         "snn_prune": "--snn-prune", "clonotypes": "--clonotypes", "clonotype_resolution": "--clonotype-resolution"}
REQUIRES = (  # (option, the option it needs): one pair is one rule
    ("cluster", "call_variants"), ("clones", "cluster"), ("neighbors", "call_variants"),
    ("snn_prune", "neighbors"), ("clonotypes", "neighbors"), ("clonotype_resolution", "clonotypes"),
)


@dataclass(frozen=True)
class AnalysisOptions:
    """The seven options as given: False or None is "not given"."""

    call_variants: bool = False
    cluster: bool = False
    clones: int | None = None
    neighbors: int | None = None
    snn_prune: float | None = None
    clonotypes: bool = False
    clonotype_resolution: float | None = None

    def given(self) -> dict:
        """The options given, by name: what the command line passes on."""
        return {k: v for k, v in vars(self).items() if v is not None and v is not False}

    def check(self, error, keywords: bool = False) -> None:
        """Raise error(message) for the first rule of REQUIRES broken: "--cluster requires --variants",
        or with `keywords` "cluster needs call_variants (--cluster requires --variants)"."""
        given = self.given()
        for option, needs in REQUIRES:
            if option in given and needs not in given:
                flags = f"{FLAGS[option]} requires {FLAGS[needs]}"
                raise error(f"{option} needs {needs} ({flags})" if keywords else flags)
